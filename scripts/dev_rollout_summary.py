"""What the rollout summaries cost (include/srbm_rti.h: srbm_rollout_*; bilevel-gait-gen_amd/rollout_summary.py), on one GPU, for 256 Config-B
instances in a closed loop with the pushes of the bench's closed-loop segment, 10 plant sub-steps, mode (0, 0.1).  Every form runs on a fresh clone of
one batch after its cold start and 2 warm-up steps, alternating, RUNS times; host clock around work that ends in a synchronisation.

    plain   the rollout with no log and no summaries (no kernel it runs differs from the parent commit's): ms per closed-loop step, the yardstick
    (a)     the rollout with a log of all its steps, the log copied to the host (srbm_step_log_get) and summarised there (srbm_rollout_fold_host)
    (b)     the same rollout in chunks: closed_loop_advance(chunk) -> fold -> step_log_reset with a log of ONE chunk, one synchronisation at the end
    (c)     the fold kernel alone on a log that is already there: one launch over all steps, and one launch per chunk; per folded step

(a) and (b) must give the same bytes (checked).  A report, not a gate: medians and spreads (max - min).
Usage: python scripts/dev_rollout_summary.py [steps [chunk [runs]]]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from srbm_loader import host, workloads, rollout_summary as rs

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
CHUNK = int(sys.argv[2]) if len(sys.argv) > 2 else 10
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
B, WARM, SUB = 256, 2, 10
CRIT = rs.criteria(z_min=0.15, tilt_max=0.5, r2_settle=0.05 ** 2, dz_settle=0.03, tilt_settle=0.02, h2_settle=1.0)


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def warmed(base, log=0):
    g = base.clone()
    g.closed_loop_advance(0, WARM, SUB, True)
    if log:
        g.step_log_enable(log)
    g.synchronize()
    return g


def plain(base):
    g = warmed(base)

    def work():
        g.closed_loop_advance(WARM, STEPS, SUB, True); g.synchronize()
    ms, _ = clock(work)
    g.close()
    return ms, None


def host_side(base, ref, mu):
    g = warmed(base, STEPS)

    def work():
        g.closed_loop_advance(WARM, STEPS, SUB, True)
        return rs.fold_host(g.L, g.step_log(), CRIT, ref, mu)             # step_log() synchronises and copies
    ms, s = clock(work)
    g.close()
    return ms, s


def chunked(base):
    g = warmed(base, CHUNK)
    rs.enable(g, CRIT)

    def work():
        rs.run(g, STEPS, CHUNK, SUB, True, first_index=WARM)
        return rs.summaries(g)
    ms, s = clock(work)
    g.close()
    return ms, s


def fold_alone(base):
    """-> (ms of one fold launch over all steps, ms of the folds of the same log chunk by chunk)"""
    g = warmed(base, STEPS)
    rs.enable(g, CRIT)
    g.closed_loop_advance(WARM, STEPS, SUB, True)
    rs.fold(g, 0, CHUNK); g.synchronize()                                   # first launch of the kernel: code object load
    rs.reset(g); g.synchronize()

    def one():
        rs.fold(g, 0, STEPS); g.synchronize()

    def by_chunk():
        for first in range(0, STEPS, CHUNK):
            rs.fold(g, first, min(CHUNK, STEPS - first))
        g.synchronize()
    ms_one, _ = clock(one)
    rs.reset(g); g.synchronize()
    ms_chunks, _ = clock(by_chunk)
    g.close()
    return ms_one, ms_chunks


def main():
    cfg = host.load_config()
    states, ees = workloads.instances(cfg, workloads.config_b_instance, B)
    base = host.BatchMPC.cold_start(cfg, states, ees, mode=(0.0, host.FAST_START_MU))
    base.plant_set_state(states)
    rng = np.random.default_rng(777)
    imp = np.zeros((B, 6))
    imp[:, 0:2] = np.clip(rng.normal(0.0, 2.5, (B, 2)), -7.5, 7.5)
    imp[:, 5] = rng.normal(0.0, 0.2, B)
    base.plant_set_push(np.full(B, 2.5 * cfg['integrator_dt']), imp)
    base.synchronize()
    ref = rs.reference_from_config(cfg, B)
    mu = np.full(B, cfg['friction_coef'])
    t = {k: [] for k in ('plain', 'a', 'b', 'c_one', 'c_chunks')}
    for r in range(RUNS):
        t['plain'].append(plain(base)[0])
        ms, sa = host_side(base, ref, mu); t['a'].append(ms)
        ms, sb = chunked(base); t['b'].append(ms)
        assert sa.tobytes() == sb.tobytes(), 'the chunked device fold and the host fold of the full log differ'
        one, chunks = fold_alone(base)
        t['c_one'].append(one); t['c_chunks'].append(chunks)
    base.close()
    T = rs.STUDY_FIELDS
    st = rs.study_host(host.lib(), sb)
    print('256 Config-B instances x %d closed-loop steps, %d sub-steps, chunk %d, %d runs; study: %d fallen, %d settled, %d with failed solves'
          % (STEPS, SUB, CHUNK, RUNS, st[T['fallen']][0], st[T['settled']][0], st[T['failed']][0]))
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = lambda k, what: print('    %-9s %-74s median %9.3f ms  spread %7.3f  per step %8.4f' % (k, what, med[k], max(t[k]) - min(t[k]), med[k] / STEPS))
    line('plain', 'rollout, no log, no summaries')
    line('a', 'rollout + full log (%.1f MB) to the host + host fold' % (8e-6 * host.STEP_LOG_DOUBLES * B * STEPS))
    line('b', 'rollout in chunks + device fold, log of one chunk (%.2f MB)' % (8e-6 * host.STEP_LOG_DOUBLES * B * CHUNK))
    line('c_one', 'fold kernel alone, one launch over all steps')
    line('c_chunks', 'fold kernel alone, one launch per chunk')
    step = med['plain'] / STEPS
    print('    fold per folded step against one closed-loop step (%.4f ms): one launch %+.3f %%, per chunk %+.3f %%;  (b) against plain %+.2f %%, (a) against plain %+.2f %%'
          % (step, 100 * med['c_one'] / STEPS / step, 100 * med['c_chunks'] / STEPS / step, 100 * (med['b'] / med['plain'] - 1), 100 * (med['a'] / med['plain'] - 1)))


if __name__ == '__main__':
    main()
