"""What the step log costs (include/srbm_rti.h: srbm_step_log_*): the same multi-step launch with and without a log, on clones of one batch after
its cold start, alternating unlogged / logged, three runs each, timed by the library's HIP events around the launch (srbm_enable_kernel_timing).

    Config B   256 instances x 100 open-loop steps in the bench's solver mode (srbm_rti_fused against srbm_rti_fused_logged)
    Config D   512 instances x 20 closed-loop steps, 10 plant sub-steps, one push per instance at 2.5 dt as bench.py draws them
               (the step queues: srbm_rti_queued_long against srbm_rti_queued_long_logged)

Every clone starts from the same state and runs 2 warm-up steps before the timed launch, so both forms solve the same QPs (the records of the
logged form are compared with nothing here: tests/test_gpu_step_log.py).  A report, not a gate: medians and spreads (max - min) of ms per step.
Usage: python scripts/dev_step_log_cost.py [runs]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from srbm_loader import host, workloads

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
WARM = 2


def timed_launch(base, closed, steps, logged):
    g = base.clone()
    if logged:
        g.step_log_enable(WARM + steps)
    adv = (lambda f, k: g.closed_loop_advance(f, k, 10, True)) if closed else g.rti_advance
    adv(0, WARM); g.synchronize()
    g.enable_kernel_timing(1)
    adv(WARM, steps); g.synchronize()
    ms = g.kernel_timings(1)[0]
    info = g.debug_launch_info()
    assert not logged or g.step_log_count() == WARM + steps
    err = int(np.bitwise_or.reduce(g.status_accumulated()[:, 0]))
    g.close()
    return ms / steps, info['kernel'], err


def protocol(name, cfg, make_inst, B, steps, closed):
    states, ees = workloads.instances(cfg, make_inst, B)
    # open loop: the bench's mode (lower start); under a plant the library makes no lower-start attempt
    base = host.BatchMPC.cold_start(cfg, states, ees, mode=None if closed else (0.0, host.FAST_START_MU))
    if closed:
        base.plant_set_state(states)
        rng = np.random.default_rng(777)
        imp = np.zeros((B, 6))
        imp[:, 0:2] = np.clip(rng.normal(0.0, 2.5, (B, 2)), -7.5, 7.5)
        imp[:, 5] = rng.normal(0.0, 0.2, B)
        base.plant_set_push(np.full(B, 2.5 * cfg['integrator_dt']), imp)
    base.synchronize()
    t, errs = {False: [], True: []}, 0
    for r in range(RUNS):
        for logged in (False, True):
            ms, kernel, err = timed_launch(base, closed, steps, logged)
            t[logged].append(ms); errs |= err
    base.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    fmt = lambda v: ' '.join('%.4f' % x for x in v)
    print('%s  %d x %d steps, kernel %s (logged: its _logged twin), error bits of all runs %d, ms per step' % (name, B, steps, kernel, errs))
    print('    unlogged  %s   median %.4f  spread %.4f' % (fmt(t[False]), med[False], max(t[False]) - min(t[False])))
    print('    logged    %s   median %.4f  spread %.4f' % (fmt(t[True]), med[True], max(t[True]) - min(t[True])))
    print('    logged / unlogged medians: %+.2f %%   (the record: %d B per solve, %.1f KB per step of this batch)'
          % (100.0 * (med[True] / med[False] - 1.0), 8 * host.STEP_LOG_DOUBLES, 8 * host.STEP_LOG_DOUBLES * B / 1e3))


protocol('Config B open loop  ', host.load_config(), workloads.config_b_instance, 256, 100, False)
protocol('Config D closed loop', host.load_config('a1_config_distr_rejection'), workloads.config_d_instance, 512, 20, True)
