"""What the MPC rate costs (include/srbm_rti.h: srbm_plant_set_period): 256 Config-B instances with the pushes of bench.py's closed-loop segment
(lin-mom xy ~ N(0, 2.5^2) truncated at 3 sigma, yaw ang-mom ~ N(0, 0.2^2), seed 777, at t = 2.5 dt; 10 plant sub-steps per period with the time
advanced), solver mode (0, 0.1).  The same 1 s of rollout at the periods dt, dt / 2 and dt / 5 -- 20, 40 and 100 solve steps in one launch --, and
one batch with the three periods mixed (instance b at PERIODS[b % 3], 40 steps: the instances then cover 2 s, 1 s and 0.4 s).

Every repetition runs on a fresh clone of one batch after its cold start, the host clock stops after one synchronisation.  One untimed repetition of
each form first, then REPS timed ones, the forms alternating.  A report, not a gate: ms per solve step (median, spread = max - min),
factorisations (IPM iterations) per solve, solves per second, lower-start attempts, solves not Solved, error bits.
Usage: python scripts/dev_mpc_period.py [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from srbm_loader import host, mpc_period, workloads

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B, SUB, MODE = 256, 10, (0.0, 0.1)


def one(base, periods, steps):
    g = base.clone()
    mpc_period.plant_set_period(g, periods)
    g.clear_status_accumulators()
    it0 = g.work_counters()[0]
    c0 = g.solver_counters()
    g.synchronize()
    t0 = time.perf_counter()
    g.closed_loop_advance(0, steps, SUB, True)
    g.synchronize()
    el = time.perf_counter() - t0
    acc, c1 = g.status_accumulated(), g.solver_counters()
    solves = int(acc[:, 1].sum())
    assert solves == B * steps, (solves, B, steps)
    out = dict(ms=1e3 * el / steps, fact=(g.work_counters()[0] - it0) / solves, rate=solves / el, low_tried=c1['low_tried'] - c0['low_tried'],
               low_failed=c1['low_failed'] - c0['low_failed'], not_solved=int(acc[:, 2].sum()), err=int(np.bitwise_or.reduce(acc[:, 0])),
               finite=bool(np.all(np.isfinite(g.plant_state()))))
    g.close()
    return out


cfg = host.load_config('a1_configuration')
dt = cfg['integrator_dt']
states, ees = workloads.instances(cfg, workloads.config_b_instance, B)
base = host.BatchMPC.cold_start(cfg, states, ees, mode=MODE)
base.plant_set_state(states)
rng = np.random.default_rng(777)
imp = np.zeros((B, 6))
imp[:, 0:2] = np.clip(rng.normal(0.0, 2.5, (B, 2)), -7.5, 7.5)
imp[:, 5] = rng.normal(0.0, 0.2, B)
base.plant_set_push(np.full(B, 2.5 * dt), imp)
base.synchronize()
PERIODS = np.array([dt, dt / 2, dt / 5])
forms = [('p = dt      ', np.full(B, PERIODS[0]), 20), ('p = dt / 2  ', np.full(B, PERIODS[1]), 40), ('p = dt / 5  ', np.full(B, PERIODS[2]), 100),
         ('mixed       ', PERIODS[np.arange(B) % 3], 40)]
res = {name: [] for name, _, _ in forms}
for rep in range(REPS + 1):
    for name, periods, steps in forms:
        r = one(base, periods, steps)
        if rep > 0:
            res[name].append(r)
base.close()
print('closed loop at an MPC period: %d Config-B instances, N = %d, dt = %g, mode %s, %d sub-steps, %d repetitions' % (B, cfg['num_nodes'], dt, MODE, SUB, REPS))
for name, _, steps in forms:
    ms = [r['ms'] for r in res[name]]
    last = res[name][-1]
    print('    %s %3d steps  ms per solve step %s  median %.3f  spread %.3f   factorisations per solve %.2f   solves per second %.0f   '
          'lower-start attempts %d (failed %d)   not Solved %d   error bits %d   plant finite %s' %
          (name, steps, ' '.join('%.3f' % v for v in ms), np.median(ms), max(ms) - min(ms), last['fact'], np.median([r['rate'] for r in res[name]]),
           last['low_tried'], last['low_failed'], last['not_solved'], last['err'], last['finite']))
