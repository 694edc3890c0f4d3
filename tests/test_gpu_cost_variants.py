"""The MPC kernels against the oracle with a final cost that is NOT the tracking cost.

Every other batch of the suite has Phi = Q and Phi_w = w, so the lines that pick the cost of node N -- `Qk = (k == N) ? s_Phi : s_Q` and `Phi_w` / `w`
of the condensing (csrc/srbm_k2_condense.hiph), the costates, the merit of the twelve candidates and the directional derivative of the update
(csrc/srbm_k4_update.hiph), the per-instance q_diag flag (csrc/srbm_capi.hip) -- and the 12 x 12 product against anything but a batch of one were
unobserved.  Here one batch holds the four cost sets of tests/cost_variants_kit.py (host checks of the sets: tests/test_cost_variants.py), interleaved
so that an instance on the diagonal path sits between instances on the full path, and runs the re-synchronised protocol of tests/gpu_protocols.py
with every assertion and every tolerance of that protocol unchanged: exported QP against the oracle's (1e-12), raw and line-searched minimiser and
states (REL_TOL), stationarity, sign, complementarity, dual objective and A'z, Armijo step, cost, foot box, knot tables.  Solver mode (0, 0): the
reference's criterion, no attempt.  No instance may leave the comparison and every solve of every set must have had its minimiser compared."""
import numpy as np
import pytest

from cost_variants_kit import SETS, cost_set
from gpu_kit import REL_TOL
from gpu_protocols import resync_protocol
from oracle_py import load_config
from srbm_loader.workloads import config_b_instance, instances

pytestmark = pytest.mark.gpu


def run(cfg, sets, per_set, steps, fused, large=None):
    """batch index b: set sets[b % len(sets)] on Config-B instance b // len(sets)"""
    B = len(sets) * per_set
    names = [sets[b % len(sets)] for b in range(B)]
    states, ees = instances(cfg, config_b_instance, [b // len(sets) for b in range(B)])
    costs = [cost_set(cfg, n) for n in names]
    r = resync_protocol(cfg, states, ees, steps=steps, qp_every=1, step_rule=False, fused=fused, large=large, costs=costs)
    c = r['counters']
    assert c['step_rule'] == 0 and c['low_tried'] == 0, c           # mode (0, 0)
    assert r['alive'] == B, r['alive']
    for s in sets:
        mine = [b for b in range(B) if names[b] == s]
        worst = {k: max(r['worst_each'][b].get(k, 0.0) for b in mine) for k in ('A', 'x', 'states', 'kkt', 'dual_obj', 'Atz', 'z_all')}
        print('cost set %s, %s, N = %d: %d solves compared, worst %s' % (s, 'fused launch' if fused else 'stand-alone kernels', cfg['num_nodes'],
                                                                         r['x_compared_each'][mine].sum(), ' '.join('%s %.2e' % kv for kv in worst.items())))
        assert np.all(r['x_compared_each'][mine] == steps), (s, r['x_compared_each'][mine])
    assert r['duals_compared_on_row_space'] == B * steps
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['states'] < REL_TOL and r['worst']['Atz'] < REL_TOL
    return r


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'standalone'])
def test_four_cost_sets_in_one_batch_match_their_oracles(fused):
    """sets A-D x Config-B instances 0..3, 8 re-synchronised steps.  fused: srbm_rti_advance(i, 1), the launch the bench times; stand-alone:
    srbm_get_real_time_update, kernels 2 and 4 launched on their own"""
    run(load_config('a1_configuration'), SETS, 4, 8, fused)


def test_full_cost_sets_on_the_large_build():
    """the LARGE build (N = 40, the configuration of the N = 40 share of tests/test_gpu_resync.py): the two sets with a full final cost, 4 steps
    through the fused launch.  Observed worst minimiser distance 7.2e-5 (set B) and 9.97e-5 (set C) of REL_TOL = 1e-4, with stationarity at 6e-10
    and the states at 6e-6: the spline variables of the 40-node QP are weakly determined; the oracle's own minimisers of
    these 32 solves are within 4e-7 of the certified ones (tests/qp_polish.py)."""
    r = run(load_config('a1_configuration', num_nodes=40), ('B', 'C'), 4, 4, True, large=True)
    assert max(r['sizes']) - 41 * 12 > 160                   # beyond the standard build's capacity
