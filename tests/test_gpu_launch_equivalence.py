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
import pytest

from gpu_protocols import run_case
from oracle_py import load_config
from srbm_loader.workloads import config_b_instance, config_d_instance

pytestmark = pytest.mark.gpu


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

