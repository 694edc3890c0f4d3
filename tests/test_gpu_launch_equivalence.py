"""A K-step launch is BITWISE the same K steps launched one at a time -- on the launches bench.py times.

bench.py times srbm_rti_advance(first, K) with K = 100 device-resident steps.  The oracle meets the device only through one-step launches
(tests/test_gpu_resync.py: srbm_rti_advance(i, 1) on a re-synchronised trajectory; tests/test_gpu_ownpath.py on the device's own path), and
a one-step launch never runs the second or later step of a launch, nor the step queues (csrc/srbm_fused.hiph: srbm_rti_queued[_long], taken
only for a batch larger than the chip and steps > 1).  This module closes that gap without the oracle: from one state after the cold start,

    reference: a chain of srbm_rti_advance(i, 1)  -- the per-instance fused kernel the resync tests hold to the oracle
    copies:    the same steps as longer launches (BatchMPC.clone copies the per-instance solver state whole, the lower-start back-off
               I.low_skip included), one launch of all steps and splits like the bench's warm-up + timed region (10 + 10, 7 + 13, 1 + 19)

and every output the library exposes must be bit-for-bit equal at the end of every launch: sizes, status and error bits, the sticky
accumulators, the solve flags, solver and work counters (batch totals and per-instance iterations), the line-search stats, primal, raw
minimiser, duals, node states and the trajectory records as bytes -- no tolerance.  So whatever the resync tests establish of a one-step
launch at a mode and a configuration holds for the multi-step launches of that mode and configuration: the solver state an instance carries
from one step to the next within a launch (the back-off of the lower-start attempts among it), the (first + s) * dt time arithmetic and the
hand-off of an instance between CUs on the step queues cannot differ from what a sequence of one-step launches does.

Each case also asserts that it covered what it exists to check: in the start_mu > 0 modes attempts were repeated and the back-off made solves
skip their attempt (the first steps after a cold start are where attempts fail in a row: docs/history.md, "attempt policies"), and the
multi-step launches of Config D took the step queues (srbm_debug_get_launch_info) while the one-step chain did not."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, config_d_instance

pytestmark = pytest.mark.gpu


def advance(g, closed, first, steps):
    if closed:
        g.closed_loop_advance(first, steps)
    else:
        g.rti_advance(first, steps)


def snapshot(g, closed):
    st, err = g.status()
    z, s = g.dual_solution()
    it = np.zeros(g.batch)
    g._chk(g.L.srbm_debug_get_instance_iters(g.h, it.ctypes.data_as(C.POINTER(C.c_double))))
    c = g.solver_counters()
    out = dict(sizes=g.sizes(), status=st, err=err, acc=g.status_accumulated(), flags=g.solve_flags(),
               solver_counters=np.array([c['solves'], c['step_rule'], c['low_tried'], c['low_failed']]), work_counters=np.array(g.work_counters()),
               instance_iters=it, stats=g.stats(), x=g.qp_solution(), x_raw=g.raw_qp_minimiser(), z=z, s=s, states=g.trajectory_states(),
               trajectory=bytes(g.get_trajectory()))
    if closed:
        out['plant'] = g.plant_state()
    return out


def assert_bitwise(a, b, where):
    for k in a:
        if isinstance(a[k], bytes):
            assert a[k] == b[k], '%s: %s differs' % (where, k)
        elif a[k].tobytes() != b[k].tobytes():
            diff = (a[k].view(np.uint8) != b[k].view(np.uint8)).reshape(len(a[k]), -1).any(axis=1) if a[k].ndim > 1 else a[k] != b[k]
            raise AssertionError('%s: %s differs at %s %s' % (where, k, 'instances' if a[k].ndim > 1 else 'entries', np.nonzero(diff)[0][:8].tolist()))


def run_case(cfg, make_inst, B, steps, mode, splits, large=None, closed=False, prepare=None):
    """cold start, then the one-step chain and the split launches from clones of the same state; returns the chain's counter deltas.
    prepare(batch): called after the cold start (e.g. a contact schedule of its own)"""
    states, ees = zip(*[make_inst(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees).reshape(B, 12)
    base = host.BatchMPC(cfg, B, large=large)
    base.set_state_trajectory_warm_start(states)
    base.set_solver_tolerances(1e-15, 1e-15, 1e-10, 200)          # the bench's settings
    base.set_solver_step_rule(*mode)
    base.create_initial_run(states, ees)
    if prepare is not None:
        prepare(base)
    if closed:                                                     # the pushes of tests/test_gpu_queue.py
        base.plant_set_state(states)
        imp = np.zeros((B, 6)); imp[::7, 0] = 0.4; imp[::11, 1] = -0.3
        base.plant_set_push(time=np.full(B, 2.5 * cfg['integrator_dt']), impulse=imp)
    base.synchronize()
    c0 = base.solver_counters()
    chain = base.clone()
    ref = []
    for i in range(steps):
        advance(chain, closed, i, 1)
        chain.synchronize()
        info = chain.debug_launch_info()
        assert info['steps'] == 1 and not info['queued'], info
        ref.append(snapshot(chain, closed))
    n_cu = info['n_cu']
    c1 = chain.solver_counters()
    chain.close()
    assert all(sum(sp) == steps for sp in splits) and any(len(sp) == 1 for sp in splits)
    queued_launches = 0
    for sp in splits:
        c = base.clone()
        first = 0
        for k in sp:
            advance(c, closed, first, k)
            c.synchronize()
            info = c.debug_launch_info()
            assert info['steps'] == k and info['queued'] == (B > n_cu and k > 1), info
            queued_launches += info['queued']
            first += k
            assert_bitwise(snapshot(c, closed), ref[first - 1], 'split %s, after step %d' % (sp, first))
        c.close()
    base.close()
    d = {k: c1[k] - c0[k] for k in c0}
    if mode[1] > 0 and not closed:                                 # (no attempts at all otherwise)
        d['skipped_attempts'] = d['solves'] - d['low_tried']
    print('launch equivalence B=%d steps=%d mode=%s closed=%d: n_cu %d, multi-step launch kernel %s, queued launches %d, chain counters %s'
          % (B, steps, mode, closed, n_cu, info['kernel'], queued_launches, d))
    assert d['solves'] == B * steps
    return dict(counters=d, n_cu=n_cu, queued_launches=queued_launches, kernel=info['kernel'], sizes=[r['sizes'] for r in ref], err=[r['err'] for r in ref])


def assert_attempts_and_back_off(d):
    # attempts were made, some of them failed and were repeated, and the back-off made later solves skip the attempt: the state that crosses
    # from step to step inside a launch was exercised
    assert d['low_tried'] > 0 and d['low_failed'] > 0 and d['low_tried'] < d['solves'], d


@pytest.mark.parametrize('mode', [(0.0, 0.1), (1e-5, 0.1), (0.0, 0.0)], ids=['lower_start', 'step_rule', 'reference'])
def test_config_b_one_launch_equals_one_step_launches(mode):
    """Config B, 256 instances (one per CU: srbm_rti_fused walks every instance through all steps) x 20 steps"""
    cfg = load_config()
    r = run_case(cfg, config_b_instance, 256, 20, mode, [(20,), (10, 10), (7, 13), (1, 19)])
    assert r['kernel'] == 'srbm_rti_fused' and r['queued_launches'] == 0
    if mode[1] > 0:
        assert_attempts_and_back_off(r['counters'])
    else:
        assert r['counters']['low_tried'] == 0


@pytest.mark.parametrize('mode', [(0.0, 0.1), (1e-5, 0.1)], ids=['lower_start', 'step_rule'])
@pytest.mark.parametrize('B,steps,splits', [(512, 12, [(12,), (6, 6), (5, 7), (1, 11)]), (600, 6, [(6,), (3, 3), (2, 4), (1, 5)])],
                         ids=['512x12', '600x6'])
def test_config_d_queued_launch_equals_one_step_launches(B, steps, splits, mode):
    """Config D (N = 50), batches larger than the chip: the multi-step launches run on the step queues (srbm_rti_queued_long); 600 instances
    leave the eight queues ragged"""
    cfg = load_config('a1_config_distr_rejection')
    r = run_case(cfg, lambda c, b: config_d_instance(c, b % 512), B, steps, mode, splits)
    assert B > r['n_cu'], r                                     # (the case exists to run the queues: a chip with more CUs than the batch would not)
    assert r['kernel'] == 'srbm_rti_queued_long' and r['queued_launches'] == sum(sum(1 for k in sp if k > 1) for sp in splits), r
    assert_attempts_and_back_off(r['counters'])


def test_config_d_queued_closed_loop_with_pushes_equals_one_step_launches():
    """srbm_closed_loop_advance on the step queues (520 instances, pushes at 2.5 dt): the plant state crosses steps too.  Under a plant the
    library makes no lower-start attempt (include/srbm_rti.h), so none is counted"""
    cfg = load_config('a1_config_distr_rejection')
    splits = [(5,), (2, 3), (1, 4)]
    r = run_case(cfg, lambda c, b: config_d_instance(c, b % 512), 520, 5, (1e-5, 0.1), splits, closed=True)
    assert 520 > r['n_cu'], r
    assert r['kernel'] == 'srbm_rti_queued_long' and r['queued_launches'] == sum(sum(1 for k in sp if k > 1) for sp in splits), r
    assert r['counters']['low_tried'] == 0 and r['counters']['step_rule'] > 0, r


def test_n40_large_build_launch_equals_one_step_launches():
    """the N = 40 share on the LARGE-capacity build (Config E's batch of 128): srbm_rti_fused_long of that build"""
    cfg = load_config(num_nodes=40)
    r = run_case(cfg, config_b_instance, 128, 6, (0.0, 0.1), [(6,), (3, 3), (1, 5)], large=True)
    assert r['kernel'] == 'srbm_rti_fused_long' and r['queued_launches'] == 0
    assert r['counters']['low_tried'] > 0, r

