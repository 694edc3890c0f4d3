"""Bitwise A/B of the RTI step between two library builds: python scripts/dev_bitwise_ab.py <parent's libsrbm_rti.so> <branch's libsrbm_rti.so>
Each library runs in its own process (SRBM_RTI_LIB).  8 seeded Config-B instances and 4 Config-D instances (N = 50: the *_long body, 3 rows per
thread): cold start in the bench's solver mode (0, 0.1), then 6 fused steps in two launches of 3 -- long enough for a repeated lower-start attempt and for
both n_u values of the schedule.  After each launch: the packed result records, the sizes, the flags of the solve, and what the condensing of the launch's last step left in every
work record (packed H, g, the compact Sig rows, sig0, n_u, error bits: host.condensed); at the end the sticky accumulators,
the solver counters and the per-instance iteration counts.  Prints what each build saw (n_u values, attempts tried / repeated) and exits 1 on any
differing byte.  For a change of the kernels that is meant to leave every result alone (scripts/README.md, identity of two builds, when the
instructions may differ)."""
import os, pickle, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('B', 'a1_configuration', 8), ('D', 'a1_config_distr_rejection', 4)]
STEPS = 6

if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
    import numpy as np
    from srbm_loader import host
    from srbm_loader import workloads
    from gpu_kit import snapshot
    out = {}
    for wl, name, B in CASES:
        cfg = host.load_config(name)
        states, ees = workloads.instances(cfg, workloads.config_b_instance if wl == 'B' else workloads.config_d_instance, B)
        g = host.BatchMPC.cold_start(cfg, states, ees, mode=(0.0, host.FAST_START_MU))
        for k in range(0, STEPS, 3):
            g.rti_advance(k, 3); g.synchronize()
            out['%s step %d: records' % (wl, k)] = g.pack_results()
            out['%s step %d: sizes' % (wl, k)] = g.sizes()
            out['%s step %d: flags' % (wl, k)] = g.solve_flags()
            cd = [host.condensed(g, b) for b in range(B)]          # what the condensing of the launch's last step left in the work records
            for key in ('packed', 'g', 'Sig', 'sig0'):
                out['%s step %d: condensed %s' % (wl, k, key)] = np.concatenate([c[key].ravel() for c in cd])
            out['%s step %d: condensed nu, err' % (wl, k)] = np.array([[c['nu'], c['err']] for c in cd])
        for key, v in snapshot(g, False).items():
            out['%s end: %s' % (wl, key)] = v
        c = g.solver_counters()
        print('%-28s %s: n_u %s  solves %d  attempts %d  repeated %d  not solved %d' % (os.path.basename(os.environ['SRBM_RTI_LIB']), wl,
              sorted({int(v) for k in range(0, STEPS, 3) for v in out['%s step %d: sizes' % (wl, k)][:, 0] - 12 * (g.N + 1)}), c['solves'], c['low_tried'], c['low_failed'],
              int(g.status_accumulated()[:, 2].sum())))
        g.close()
    pickle.dump(out, open(sys.argv[2], 'wb'))
else:
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    got = []
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate(sys.argv[1:]):
            f = os.path.join(d, '%d.pkl' % i)
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), '--child', f], env=dict(os.environ, SRBM_RTI_LIB=os.path.abspath(lib)))
            if rc != 0:
                sys.exit('the run of %s ended with %d: no further run' % (lib, rc))          # (after a fault nothing more is started on the GPU)
            got.append(pickle.load(open(f, 'rb')))
    a, b = got
    bad = [k for k in a if (a[k] != b[k] if isinstance(a[k], bytes) else a[k].tobytes() != b[k].tobytes())]
    print('%d arrays compared, %d differ%s' % (len(a), len(bad), ': ' + '; '.join(bad[:12]) if bad else ''))
    sys.exit(1 if bad or set(a) != set(b) else 0)
