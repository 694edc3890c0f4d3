"""Bitwise A/B of the whole-body plants and the touch-down rule between library builds:
python scripts/dev_ab_controller.py [--large] build_ab/libA.so build_ab/libB.so ...
Each library runs in its own process (SRBM_RTI_LIB, or SRBM_RTI_LIB_LARGE with --large) on the worlds of the GPU tests -- 4 Config-B instances after
one cold start (test_gpu_controller_rollout.World), the plants' settings and grounds of tests/wb_torque_plant_kit.py, wb_ground_plant_kit.py and
contact_feedback_kit.py -- and dumps, per case, q, v, the contact state, the feedback record, the whole tick log, the step log, the trajectories'
node states and status / err at the end (the stand-alone cases: every output of the entry).  The parent compares every array of every library with
the first one's byte for byte and exits 1 on a difference; nothing is started after a child that ends non-zero.  The cases:
  a  srbm_controller_advance, plant kind 0, logged and unlogged, instance 2 pushed inside tick 3 and instance 0 at the boundary of ticks 5 and 6
  b  kind 1 with the feet held, S = 1 and 3, bodies of the plant's own on the odd instances, instance 3 limited to 8 Nm (its joints clamp), the
     pushes of (a); logged and unlogged
  c  kind 1 on the ground of test_gpu_wb_ground_plant.py's rollouts (feet in the air, sticking, slipping), S = 1 and 3; logged and unlogged
  d  the ground with contact feedback on, on the raised ground of test_gpu_contact_feedback.py (which moves touch-downs), ticks 20 .. 31 of 10 ms
     with an update every 3, S = 1, 3 and the kit's 4; then srbm_adjust_for_current_contacts on a clone with the flags the ground ended with, and on
     the cold-started batch at t = 0.24 with every foot flagged (the swing feet are 60 ms from their touch-down)
  s  srbm_wb_forward_dynamics and srbm_wb_ground_dynamics on the kits' solve cases, srbm_wb_fd_step_dev and srbm_wb_ground_step_dev with sol_out
     on their step cases (zero control actions, a clamped joint, pushes at both ends of the tick and inside it), S = 1 and 3
a, b, c: 10 ticks with an update every 5, at ticks of 1 ms and again at the tests' 10 ms (at 1 ms the feet hardly reach the ground in 10 ticks)."""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
    import numpy as np
    from srbm_loader import host
    from srbm_loader.controller_rollout import ControllerRollout, PLANT_TORQUE_DRIVEN, decode_ground_word
    from srbm_loader.workloads import config_b_instance, instances
    import controller_rollout_kit as kit
    import wb_torque_plant_kit as fd
    import wb_ground_plant_kit as gk
    import contact_feedback_kit as fk
    from test_gpu_controller_rollout import World, Dev
    from test_gpu_wb_ground_plant import own_bodies, rollout_ground
    from test_gpu_contact_feedback import K0, NT, TPU as TPU_FB
    large = os.environ['AB_LARGE'] == '1'
    B, N, TPU = kit.B, 10, 5

    class LibWorld(World):
        """World (its fresh()) on the build under test: the same batch, cold-started with `large`"""
        def __init__(self):
            self.cfg = host.load_config('a1_configuration')
            self.model = kit.Model(self.cfg)
            self.states, self.ees = instances(self.cfg, config_b_instance, B)
            self.base = host.BatchMPC.cold_start(self.cfg, self.states, self.ees, large=large)
            self.q0 = np.tile(np.array(self.cfg['init_config'], float), (B, 1))
            qd, vd, _, st = self.base.clone().get_targets_from_traj(0.0, self.q0)
            assert np.all(st == 0)
            self.q, self.v = kit.first_measured(qd, vd)

    w = LibWorld()
    assert w.base.large == large
    out, notes = {}, []

    def dump(tag, g, R, ground=False):
        g.synchronize()
        out[tag + '.q'], out[tag + '.v'] = R.state()
        out[tag + '.cs'], out[tag + '.fb'] = R.contact_state(), R.contact_feedback()
        if R.tick_log_count():
            out[tag + '.ticks'] = log = R.tick_log()
            if ground:
                word = decode_ground_word(log[:, :, 63])
                notes.append('%s: foot-ticks in contact %d, slipping %d; feedback moved %d' % (
                    tag, int(word['in_contact'].sum()), int(word['slipping'].sum()), int(out[tag + '.fb'][:, :, 0].sum())))
            else:
                notes.append('%s: pushed ticks %d, clamped joint-ticks %d' % (tag, int((log[:, :, 5].astype(int) & 1).sum()), int(log[:, :, 58].sum())))
        out[tag + '.steps'] = g.step_log()
        out[tag + '.states'] = g.trajectory_states()
        out[tag + '.trajectory'] = fk.traj_bytes(g)
        out[tag + '.status'], out[tag + '.err'] = g.status()

    lists, models = own_bodies(w.cfg)
    act = (np.full((B, 12), fd.KP), np.full((B, 12), fd.KD), np.tile(np.asarray(w.cfg['torque_bounds'], float), (B, 1)))
    act[2][3] = 8.0
    ground = rollout_ground(w)
    for h in (1e-3, kit.TICK_DT):
        push_time = np.full(B, -1.0); push_time[2] = 3.5 * h; push_time[0] = 6 * h
        impulse = np.zeros((B, 6)); impulse[2] = kit.IMPULSE; impulse[0] = -kit.IMPULSE
        for logged in (True, False):
            def fresh():
                g, R = w.fresh(tick_log=N if logged else 0, step_log=4, push=False)
                g.plant_set_push(push_time, impulse)
                return g, R
            tail = '.h%g.%s' % (h, 'logged' if logged else 'unlogged')
            g, R = fresh()
            R.advance(0, N, TPU, h)
            dump('a' + tail, g, R)
            for S in (1, 3):
                g, R = fresh()
                R.set_plant(PLANT_TORQUE_DRIVEN, *act, S)
                R.set_plant_bodies(*fd.bodies_arrays(lists))
                R.advance(0, N, TPU, h)
                dump('b.S%d' % S + tail, g, R)
                g, R = fresh()
                R.set_plant(PLANT_TORQUE_DRIVEN, *act, S)
                R.set_plant_bodies(*fd.bodies_arrays(lists))
                R.set_ground(ground)
                R.advance(0, N, TPU, h)
                dump('c.S%d' % S + tail, g, R, ground=True)
    # d: contact feedback on a raised ground
    gw = fk.GroundWorld(w)
    raised = fk.raised_ground(gw, K0)
    for S in (1, 3, fk.SUB):
        g, R = gw.fresh(K0, raised, feedback=1, tick_log=NT, step_log=4)
        R.set_plant(PLANT_TORQUE_DRIVEN, *gw.act, S)
        R.advance(K0, NT, TPU_FB, fk.H)
        dump('d.S%d' % S, g, R, ground=True)
        c = g.clone()
        c.adjust_for_current_contacts((K0 + NT) * fk.H, (R.contact_state()[:, :, 0] != 0).astype(np.int32))
        c.synchronize()
        out['d.S%d.adjust.trajectory' % S] = fk.traj_bytes(c)
        out['d.S%d.adjust.status' % S], out['d.S%d.adjust.err' % S] = c.status()
    c = w.base.clone()
    before = fk.traj_bytes(c).copy()
    c.adjust_for_current_contacts(0.24, np.ones((B, 4), np.int32))
    c.synchronize()
    out['d.adjust.trajectory'] = fk.traj_bytes(c)
    out['d.adjust.status'], out['d.adjust.err'] = c.status()
    notes.append('d.adjust: the rule moved knots: %s' % (not np.array_equal(before, out['d.adjust.trajectory'])))
    # s: the stand-alone entries
    g = host.BatchMPC(w.cfg, B, large=large)
    R = ControllerRollout(g)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    for i, (q, v, tau, contact) in enumerate(fd.solve_cases(w.cfg)):
        out['s.fd%d.sol' % i], out['s.fd%d.status' % i] = R.forward_dynamics(q, v, tau, contact)
    R.set_plant(PLANT_TORQUE_DRIVEN, *fd.step_actuators(w.cfg), 1)
    for i, c in enumerate(gk.solve_cases(w.cfg, models)):
        R.set_ground(c['ground'])
        out['s.gd%d.sol' % i], out['s.gd%d.cs' % i], out['s.gd%d.status' % i] = R.ground_dynamics(c['q'], c['v'], c['tau'], c['cs'])
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, *fd.step_actuators(w.cfg), S)
        for pushed in (False, True):
            for i, (c, cg) in enumerate(zip(fd.step_cases(w.cfg, kit.TICK_DT), gk.step_cases(w.cfg, models, kit.TICK_DT))):
                g.plant_set_push(c['push_time'], c['impulse']) if pushed else g.plant_set_push()
                tag = 's.step%d.S%d.%s' % (i, S, 'pushed' if pushed else 'plain')
                d = dict(q=Dev(c['q']), v=Dev(c['v']), ctl=Dev(c['control']), con=Dev(c['contact']), st=Dev(c['status']), sol=Dev(np.zeros((B, 30))))
                R.fd_step_dev(c['k'], kit.TICK_DT, d['q'].p.value, d['v'].p.value, d['ctl'].p.value, d['con'].p.value, d['st'].p.value, d['sol'].p.value)
                g.synchronize()
                out[tag + '.fd.q'], out[tag + '.fd.v'], out[tag + '.fd.sol'] = d['q'].get(), d['v'].get(), d['sol'].get()
                R.set_ground(cg['ground'])
                d = dict(q=Dev(cg['q']), v=Dev(cg['v']), cs=Dev(cg['cs']), ctl=Dev(cg['control']), st=Dev(cg['status']), sol=Dev(np.zeros((B, 30))))
                R.ground_step_dev(cg['k'], kit.TICK_DT, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value, d['sol'].p.value)
                g.synchronize()
                out[tag + '.ground.q'], out[tag + '.ground.v'], out[tag + '.ground.sol'] = d['q'].get(), d['v'].get(), d['sol'].get()
                out[tag + '.ground.cs'] = d['cs'].get()
    np.savez(os.environ['AB_OUT'], **out)
    print('%s: %d arrays' % (os.path.basename(os.environ['AB_LIB']), len(out)))
    print('\n'.join('  ' + n for n in notes))
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
        assert sorted(dumps[0].files) == sorted(dumps[i].files)
        for k in dumps[0].files:
            a, b = dumps[0][k], dumps[i][k]
            same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
            bad += not same
            if not same:
                print('%-40s %-16s DIFFERENT: %d entries' % (k, a.shape, (a != b).sum() if a.shape == b.shape else -1))
    print('%s%s: %d arrays each, %s' % (' vs '.join(os.path.basename(l) for l in libs), ' (LARGE)' if large else '', len(dumps[0].files),
                                        'all bitwise equal' if bad == 0 else '%d differ' % bad))
    sys.exit(1 if bad else 0)
