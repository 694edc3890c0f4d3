"""What the tick summaries cost (srbm_tick_summary_fold), by the protocol of dev_controller_rollout.py, on its row (e) at S = 4:
256 Config-B instances after the cold start, the torque-driven plant on the compliant ground, 200 ticks of 1 ms, an MPC update every 50 ticks, the
variants in turn on fresh clones, three runs each; medians and spreads.
  (a) logged     srbm_controller_advance, all ticks in one call into a tick log of all ticks (nothing folded): the rollout as it was
  (b) chunked    tick_summary.run in chunks of 50 and of 10 ticks, a tick log of one chunk, every chunk folded; beside (a) this is what chunking and
                 folding cost per tick.  The summaries of every variant are compared, bit for bit, with the host fold of (a)'s log
  (c) fold       the fold kernel alone on (a)'s log: one launch over the 200 slots, and 20 launches of 10 slots; microseconds per folded tick
With `--logged-only` only (a) runs: the row the parent's tree can run too.
Every launch is under a time limit of its own (an alarm re-armed per call: a launch or a wait that does not return ends the process).
Prints one JSON line."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srbm_loader import host
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS, PLANT_TORQUE_DRIVEN
from srbm_loader.workloads import config_b_instance, instances

B, TICKS, TPU, DT, LIMIT_S, SUB = 256, 200, 50, 1e-3, 60.0, 4
CHUNKS = (50, 10)
LOGGED_ONLY = '--logged-only' in sys.argv
RUNS = int(next((a for a in sys.argv[1:] if a.isdigit()), 3))


def main():
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    cfg = host.load_config('a1_configuration')
    states, ees = instances(cfg, config_b_instance, B)
    signal.setitimer(signal.ITIMER_REAL, 300.0)
    base = host.BatchMPC.cold_start(cfg, states, ees)
    q_init = np.tile(np.array(cfg['init_config'], float), (B, 1))
    q0, v0, _, st = base.clone().get_targets_from_traj(0.0, q_init)          # the plant starts on the targets of tick 0
    kp, kd, lim = np.full(12, 20.0), np.full(12, 0.5), np.asarray(cfg['torque_bounds'], float)
    ground = None

    def fresh(tick_log, with_ground=True):
        g = base.clone()
        R = ControllerRollout(g)
        R.reset(q_init); R.set_state(q0, v0)
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, SUB)
        if with_ground:
            R.set_ground(ground)
        R.tick_log_enable(tick_log)
        return g, R

    def timed(g, fn, per):
        g.synchronize()
        tb = time.perf_counter()
        fn()
        g.synchronize()
        return (time.perf_counter() - tb) / per

    # the plane 3 mm above each instance's lowest foot of the first tick, as dev_controller_rollout.py sets it
    g, R = fresh(1, with_ground=False)
    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
    R.advance(0, 1, TPU, DT)
    ground = np.zeros((B, 8))
    ground[:, 0] = R.tick_log()[0][:, TICK_LOG_FIELDS['foot_heights']].min(axis=1) + 0.003
    ground[:, 1:6] = [2e4, 100.0, 0.7, 1e4, 50.0]
    g.close()

    res = {'logged': []}
    info = {}
    if not LOGGED_ONLY:
        from srbm_loader import tick_summary as ts
        res.update({'chunk_%d' % c: [] for c in CHUNKS})
        res.update({'fold_us_per_tick_one_launch': [], 'fold_us_per_tick_launches_of_10': []})
        crit = ts.criteria(z_min=0.15, tilt_max=0.5, r2_settle=0.02 ** 2, dz_settle=0.02, tilt_settle=0.01, v2_settle=0.1 ** 2)
        ref = ts.reference_from_config(cfg, B)
    for run in range(RUNS):
        g, R = fresh(TICKS + 3)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        R.advance(0, 3, TPU, DT)                                              # warm-up: three ticks
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        res['logged'].append(1e3 * timed(g, lambda: R.advance(3, TICKS, TPU, DT), TICKS))
        info['finite'] = bool(np.all(np.isfinite(R.state()[0])))
        if LOGGED_ONLY:
            g.close()
            continue
        log = R.tick_log(3, TICKS)
        want = ts.fold_host(g.L, log, crit, ref)
        # (c) the fold kernel alone, on the log the rollout left
        ts.enable(g, crit, ref)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        ts.fold(g, 3, TICKS)                                                  # warm-up, and the comparison
        same = [bool(ts.summaries(g).tobytes() == want.tobytes())]
        ts.reset(g)
        res['fold_us_per_tick_one_launch'].append(1e6 * timed(g, lambda: ts.fold(g, 3, TICKS), TICKS))
        ts.reset(g)
        res['fold_us_per_tick_launches_of_10'].append(1e6 * timed(g, lambda: [ts.fold(g, 3 + s, 10) for s in range(0, TICKS, 10)], TICKS))
        same.append(bool(ts.summaries(g).tobytes() == want.tobytes()))
        g.close()
        # (b) chunked and folded
        for c in CHUNKS:
            g, R = fresh(c)
            ts.enable(g, crit, ref)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            ts.fold(g, 0, 3)
            ts.reset(g)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res['chunk_%d' % c].append(1e3 * timed(g, lambda: ts.run(R, TICKS, c, TPU, DT, first_tick=3), TICKS))
            same.append(bool(ts.summaries(g).tobytes() == want.tobytes()))
            g.close()
        info['summaries_equal_the_host_fold'] = same
        info['study'] = [float(x) for x in ts.study_host(host.lib(), want)]
    signal.setitimer(signal.ITIMER_REAL, 0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps(dict(batch=B, ticks=TICKS, ticks_per_update=TPU, tick_dt=DT, substeps=SUB, runs=RUNS, units='ms per tick; fold_*: us per folded tick',
                          per_tick_runs=res, per_tick_median=med, spread={k: float(max(v) - min(v)) for k, v in res.items()}, **info)))


if __name__ == '__main__':
    main()
