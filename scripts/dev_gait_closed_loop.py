"""What the closed loop with the gait step costs (include/srbm_rti.h: srbm_gait_closed_loop_advance): 256 instances with the values and the
gait_opt_freq of bench.py's `gait` segment (Config C: a1_gait_opt_config at N = 20, dt = 0.05, every solve to the gap criterion, F = 5), 30 runs after
the cold start, one push per instance at 2.5 dt, 4 plant sub-steps with the time advanced.  Three forms over the same runs 1..30:

    (a) the entry in one call            plain stretches as multi-step plant launches
    (b) the entry one run per call       every run a one-step launch (what (a) would be without the stretches)
    (c) srbm_gait_rti_advance            the open-loop protocol of the parent: no plant, no pushes -- the baseline

Every repetition runs on a fresh clone of one batch after its cold start, the calls are queued without waiting and the host clock stops after ONE
synchronisation at the end.  One untimed repetition of each form first (code objects, the candidate batch's first launches), then REPS timed ones,
the forms alternating.  A report, not a gate: ms per run, median and spread (max - min).
Usage: python scripts/dev_gait_closed_loop.py [reps]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from srbm_loader import gait_rollout, host, workloads

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B, RUNS, FREQ, SUB = 256, 30, 5, 4


def one(base, form):
    g = base.clone()
    gait = host.BatchGaitOptimizer(g)
    roll = gait_rollout.GaitRollout(g, gait)
    g.synchronize()
    t0 = time.perf_counter()
    if form == 'a':
        roll.advance(1, RUNS, FREQ, SUB, True)
    elif form == 'b':
        for r in range(1, RUNS + 1):
            roll.advance(r, 1, FREQ, SUB, True)
    else:
        gait.rti_advance(1, RUNS, FREQ)
    g.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / RUNS
    acc = g.status_accumulated()
    out = dict(ms=ms, err=int(np.bitwise_or.reduce(acc[:, 0])), not_solved=int(acc[:, 2].sum()), searched=int((roll.line_search_result()[0] >= 0).sum()),
               plant=g.plant_state(), states=g.trajectory_states())
    gait.close(); g.close()
    return out


cfg = host.load_config('a1_gait_opt_config', num_nodes=20, integrator_dt=0.05)
states, ees = workloads.instances(cfg, workloads.config_c_instance, B)
base = host.BatchMPC.cold_start(cfg, states, ees, mode=(0.0, 0.0))
base.plant_set_state(states)
rng = np.random.default_rng(777)
imp = np.zeros((B, 6))
imp[:, 0:2] = np.clip(rng.normal(0.0, 1.0, (B, 2)), -3.0, 3.0)
imp[:, 5] = rng.normal(0.0, 0.1, B)
base.plant_set_push(np.full(B, 2.5 * cfg['integrator_dt']), imp)
base.clear_status_accumulators()
base.synchronize()
forms = ('a', 'b', 'c')
res = {f: [] for f in forms}
for rep in range(REPS + 1):
    for f in forms:
        r = one(base, f)
        if rep > 0:
            res[f].append(r)
base.close()
names = {'a': '(a) one call            ', 'b': '(b) one run per call    ', 'c': '(c) open loop (baseline)'}
print('closed loop with the gait step: %d instances, N = %d, runs 1..%d, gait_opt_freq %d, %d sub-steps; ms per run, %d repetitions' % (B, cfg['num_nodes'], RUNS, FREQ, SUB, REPS))
for f in forms:
    ms = [r['ms'] for r in res[f]]
    print('    %s  %s   median %.3f  spread %.3f   error bits %d, solves not Solved %d, instances that searched at run %d: %d' %
          (names[f], ' '.join('%.3f' % v for v in ms), np.median(ms), max(ms) - min(ms), np.bitwise_or.reduce([r['err'] for r in res[f]]),
           res[f][-1]['not_solved'], RUNS, res[f][-1]['searched']))
same = all(np.array_equal(res['a'][-1][k], res['b'][-1][k]) for k in ('plant', 'states'))
print('    (a) and (b) end bitwise equal: %s;  (a) / (b) medians: %+.2f %%' %
      (same, 100.0 * (np.median([r['ms'] for r in res['a']]) / np.median([r['ms'] for r in res['b']]) - 1.0)))
