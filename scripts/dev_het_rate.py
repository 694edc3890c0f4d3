"""Rate of a heterogeneous Config-B batch (every instance its own mass, inertia, friction, force bound, force cost, Q and target:
workloads.heterogeneous_configs through BatchMPC.from_configs) against the uniform Config-B batch of the same size, in the bench's solver mode
(step rule 0, start_mu 0.1): 10 cold-start solves, 5 warm-up steps, five 20-step launches timed one by one.  A report, not a gate: the
heterogeneous batch solves different QPs, so its IPM iteration count (printed) differs.  Usage: python scripts/dev_het_rate.py [batch]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from srbm_loader import host, workloads

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cfg = host.load_config()
het = workloads.heterogeneous_configs(cfg, [cfg['Q_srbd_diag'], host.load_config('a1_config_distr_rejection')['Q_srbd_diag']], B)
for name, cfgs in (('uniform', [cfg] * B), ('heterogeneous', het)):
    states, ees = workloads.instances(cfgs, workloads.config_b_instance, B)
    g = host.BatchMPC.cold_start(cfg if name == 'uniform' else cfgs, states, ees, mode=(0.0, 0.1))
    g.rti_advance(0, 5); g.synchronize()
    w = []
    for k in range(5):
        ta = time.perf_counter(); g.rti_advance(5 + 20 * k, 20); g.synchronize(); w.append((time.perf_counter() - ta) / 20)
    acc = g.status_accumulated()
    med = sorted(w)[2]
    print('%-13s B=%d  ms/step %s  median %.3f  -> %.1f k instance-steps/s  IPM iters/solve %.2f  not solved %d  err bits %d'
          % (name, B, ' '.join('%.3f' % (v * 1e3) for v in w), med * 1e3, B / med / 1e3, g.stats()[:, 4].mean(), int(acc[:, 2].sum()),
             int(np.bitwise_or.reduce(acc[:, 0]))))
    g.close()
