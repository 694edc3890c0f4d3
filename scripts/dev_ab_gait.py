"""Bitwise A/B of the gait step between library builds: python scripts/dev_ab_gait.py [--large] build_ab/libA.so build_ab/libB.so ...
Each library runs in its own process (SRBM_RTI_LIB, or SRBM_RTI_LIB_LARGE with --large) on 32 seeded Config-B instances after a cold start and
three RTI steps, and dumps the sensitivity, the gradient with its valid flags, the LP result and step, the dense parameter partials of one contact
time, and the contact times and node states after srbm_gait_rti_advance over two gradient steps and a line search.  The parent compares every
array of every library with the first one's byte for byte and exits 1 on a difference.  (Config B has n_u = 120: all of the LU in LDS in the
standard build, eight elimination steps on the copy in L2 with --large.)"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
    import numpy as np
    from srbm_loader import host
    from srbm_loader import workloads
    large = os.environ['AB_LARGE'] == '1'
    cfg = host.load_config()
    B, dt = 32, cfg['integrator_dt']
    states, ees = workloads.instances(cfg, workloads.config_b_instance, B)
    g = host.BatchMPC.cold_start(cfg, states, ees, mode=(0.0, 0.0), large=large)
    g.rti_advance(0, 3); g.synchronize()
    out = {'status': g.status()[0], 'x': g.qp_solution()}
    gait = host.BatchGaitOptimizer(g)
    gait.set_contact_times_from_trajectory()
    gait.compute_sensitivity()
    out['sensitivity'] = gait.sensitivity()
    gait.compute_gradient()
    out['gradient'], out['valid'] = gait.gradient()
    gait.optimize_contact_times(2 * dt)
    out['lp_status'], out['lp_pred'] = gait.lp_result()
    out['lp_step'] = gait.step()
    out['pp_dA'], out['pp_dG'], out['pp_db'], out['pp_dh'] = g.param_partials(0, 0, 1)
    gait.rti_advance(3, 7, 5); g.synchronize()            # runs 3 .. 9: gradient + LP at 4 and 9, line search at 5
    gait.set_contact_times_from_trajectory()
    out['contact_times'], out['contact_counts'] = gait.contact_times()
    out['states_after'] = g.trajectory_states()
    out['status_after'], out['err_after'] = g.status()
    np.savez(os.environ['AB_OUT'], **out)
    print('%-28s n_u %d  solved %d of %d  gradient valid %d  LP solved %d  after the gait steps: solved %d, err bits %d' % (
        os.path.basename(os.environ['AB_LIB']), int(g.sizes()[0, 0]) - (cfg['num_nodes'] + 1) * 12, int((out['status'] == 0).sum()), B,
        int(out['valid'].sum()), int((out['lp_status'] == 0).sum()), int((out['status_after'] == 0).sum()), int(np.bitwise_or.reduce(out['err_after']))))
else:
    import numpy as np
    args = sys.argv[1:]
    large = '--large' in args
    libs = [a for a in args if a != '--large']
    tmp = tempfile.mkdtemp()
    dumps = []
    for i, lib in enumerate(libs):
        path = os.path.join(tmp, 'ab%d.npz' % i)
        env = dict(os.environ, AB_LARGE='1' if large else '0', AB_OUT=path, AB_LIB=lib)
        env['SRBM_RTI_LIB_LARGE' if large else 'SRBM_RTI_LIB'] = os.path.abspath(lib)
        if subprocess.call([sys.executable, os.path.abspath(__file__), '--child'], env=env) != 0:
            sys.exit(2)
        dumps.append(np.load(path))
    bad = 0
    for i in range(1, len(libs)):
        for k in dumps[0].files:
            a, b = dumps[0][k], dumps[i][k]
            same = a.shape == b.shape and a.tobytes() == b.tobytes()
            bad += not same
            print('%-16s %-14s %s' % (k, a.shape, 'bitwise equal' if same else 'DIFFERENT: %d entries, max |a - b| %.3g' % ((a != b).sum(), np.nanmax(np.abs(a - b)))))
    print('%s: %s' % (' vs '.join(os.path.basename(l) for l in libs), 'all arrays bitwise equal' if bad == 0 else '%d arrays differ' % bad))
    sys.exit(1 if bad else 0)
