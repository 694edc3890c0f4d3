"""End-to-end parity on the IPM paths the other GPU tests do not reach: the compact dense state rows read from L2 instead of LDS (sig_lds = 0 in
csrc/srbm_k3_rows.hiph: eval_rows_prep, the un-fused branch of gt_apply; srbm_k3_normal.hiph: the W.Sig reads of the sparse assembly), horizons beyond N = 40 in the
LARGE build (N = 100: more than 2048 inequality rows, the fifth of the K3_RPT register slots per thread live), and the LARGE build's capacity
guard.  Each case first asserts that it takes the branch it exists for: the placement of its dense rows through srbm_debug_dense_row_placement
(the function k3_make_smem decides with; tests/test_dense_row_placement.py pins it on the CPU), n_u and wc = n_force / 3 from the oracle's sizes.

Against the oracle through the re-synchronised protocol of tests/test_gpu_resync.py (assembled QP <= 1e-12, minimiser < REL_TOL, equal sizes, no
error bits), and a K-step launch against its one-step launches, bit for bit (tests/test_gpu_launch_equivalence.py)."""
import numpy as np
import pytest

from gpu_kit import REL_TOL
from gpu_protocols import resync_protocol, run_case
from oracle_py import first_rti_sizes, load_config
from srbm_loader import host
from srbm_loader.workloads import EE_NOMINAL, config_b_instance, config_d_instance, instances

pytestmark = pytest.mark.gpu
# Contact times 0.22 s apart on Config D's horizon: at or above the gait LP's lower bound on a phase (MIN_TIME = 0.2), so the gait step can
# produce this schedule on its own; n_u stays 148 over five steps (at 0.2 s a seventh contact time per foot enters the window at the second step:
# n_u 176, beyond the standard build's 160)
PHASE_D = 0.22
PHASE_OVERFLOW = 0.2


def placements(N, shapes, large=False):
    """the dense-row placement of every (n, n_force) seen"""
    return {host.dense_row_placement(N, n - 12 * (N + 1), nf // 3, large) for n, nf in shapes}


def device_shapes(r):
    """(n, n_force) of every instance after every step of a run_case chain (srbm_get_sizes: columns 0 and 4)"""
    return {(int(sz[b, 0]), int(sz[b, 4])) for sz in r['sizes'] for b in range(sz.shape[0])}


def set_phases(g, phase):
    """the device's own contact schedule: contact times `phase` apart, as many per foot as the cold start left (srbm_update_contact_times)"""
    arr = np.zeros((g.batch, 4, 8))
    for b in range(g.batch):
        kg = g.knots(b)
        for e in range(4):
            k = int(np.sum(kg['kinds'][e, :kg['nk'][e]] <= 1))
            arr[b, e, :k] = phase * np.arange(k)
    g.update_contact_times(arr)


# ---- 1. standard build, Config D's horizon (N = 50, dt = 0.02) with 0.22 s phases: n_u 148, the dense rows in L2 ----
L2_D = (46, 0, False)           # 46 of the 94 rows would fit in the window's tail, none behind the map: every pass reads them from L2


def config_d_short_phases():
    cfg = load_config('a1_config_distr_rejection')
    nu, wc, _ = first_rti_sizes(cfg, PHASE_D)
    assert (nu, wc) == (148, 40)
    assert host.dense_row_placement(50, nu, wc) == L2_D
    return cfg, nu


@pytest.mark.parametrize('fused', [False, True], ids=['per_phase_launches', 'fused_one_step_launches'])
def test_dense_rows_from_l2_standard_build_against_the_oracle(fused):
    cfg, nu = config_d_short_phases()
    B, steps = 16, 5
    states, ees = instances(cfg, config_d_instance, B)
    r = resync_protocol(cfg, states, ees, steps=steps, qp_every=1, fused=fused, contact_phase=PHASE_D)
    print('dense rows from L2, standard build, Config D 0.22 s phases %s 16 x 5: alive' % ('fused' if fused else 'per phase'), r['alive'],
          'shapes', sorted(r['shapes']), 'minimisers compared %d of %d solves' % (r['x_compared'], r['total']), 'worst', r['worst'])
    assert r['alive'] == B and r['total'] == B * steps
    assert r['sizes'] == {51 * 12 + nu}, r['sizes']
    assert placements(50, r['shapes']) == {L2_D}                       # every compared solve took the L2 branch
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    assert r['x_compared'] >= B, r['x_compared']


def test_dense_rows_from_l2_standard_build_k_step_launch_equals_one_step_launches():
    """the fused kernel of the standard build over five steps with the dense rows in L2: a 5-step launch and 2 + 3 are bitwise the 1-step chain"""
    cfg, nu = config_d_short_phases()
    r = run_case(cfg, config_d_instance, 16, 5, (0.0, 0.1), [(5,), (2, 3), (1, 4)], prepare=lambda g: set_phases(g, PHASE_D))
    assert r['kernel'] == 'srbm_rti_fused_long' and r['queued_launches'] == 0, r
    shapes = device_shapes(r)
    assert {n - 51 * 12 for n, _ in shapes} == {nu}, shapes
    assert placements(50, shapes) == {L2_D}                            # on the device's own path too, at every step
    assert all(np.all(e == 0) for e in r['err'])


# ---- 2. LARGE build beyond N = 40: N = 100 (dense rows in L2, > 2048 inequality rows) and N = 75 (dense rows in LDS) ----
def large_case(N):
    cfg = load_config(num_nodes=N, integrator_dt=0.02)
    nu, wc, n_ineq = first_rti_sizes(cfg)
    return cfg, nu, wc, n_ineq


L2_100 = (0, 136, False)        # 136 of 194 rows fit behind the map: L2


def test_n100_large_build_against_the_oracle():
    cfg, nu, wc, n_ineq = large_case(100)
    assert (nu, wc) == (204, 56) and n_ineq == 2392 and n_ineq > 2048          # rows >= 2048: the fifth register slot of K3_RPT = 6 is live
    assert host.dense_row_placement(100, nu, wc, True) == L2_100
    B, steps = 4, 3
    states, ees = instances(cfg, config_b_instance, B)
    # the bench's headline mode (every solve ends by the reference's gap criterion): the duals are then held to REL_TOL on the row space
    r = resync_protocol(cfg, states, ees, steps=steps, qp_every=1, fused=True, large=True, step_rule=False, start_mu=host.FAST_START_MU)
    print('N = 100, LARGE build, 4 x 3 through the fused launch: alive', r['alive'], 'shapes', sorted(r['shapes']),
          'minimisers compared %d of %d solves' % (r['x_compared'], r['total']), 'worst', r['worst'])
    assert r['alive'] == B and r['total'] == B * steps
    assert 101 * 12 + nu in r['sizes'], r['sizes']
    assert all(not p[2] for p in placements(100, r['shapes'], True)), r['shapes']
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    assert r['x_compared'] >= B, r['x_compared']


def test_n100_large_build_k_step_launch_equals_one_step_launches():
    cfg, nu, wc, _ = large_case(100)
    assert host.dense_row_placement(100, nu, wc, True) == L2_100
    r = run_case(cfg, config_b_instance, 4, 4, (0.0, 0.1), [(4,), (1, 3)], large=True)
    assert r['kernel'] == 'srbm_rti_fused_long' and r['queued_launches'] == 0, r
    shapes = device_shapes(r)
    assert nu in {n - 101 * 12 for n, _ in shapes}, shapes
    assert all(not p[2] for p in placements(100, shapes, True)), shapes     # the dense rows in L2 at every step
    assert all(np.all(e == 0) for e in r['err'])


def test_n75_large_build_dense_rows_in_lds_against_the_oracle():
    cfg, nu, wc, _ = large_case(75)
    assert (nu, wc) == (172, 48) and nu > 160
    assert host.dense_row_placement(75, nu, wc, True) == (0, 144, True)        # all 144 rows behind the map
    B, steps = 4, 3
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=steps, qp_every=1, fused=True, large=True)
    print('N = 75, LARGE build, 4 x 3 through the fused launch: alive', r['alive'], 'shapes', sorted(r['shapes']),
          'minimisers compared %d of %d solves' % (r['x_compared'], r['total']), 'worst', r['worst'])
    assert r['alive'] == B and r['total'] == B * steps
    assert 76 * 12 + nu in r['sizes'], r['sizes']
    assert all(p[2] for p in placements(75, r['shapes'], True)), r['shapes']  # in LDS at every step (n_u 172 and 176)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    assert r['x_compared'] >= B, r['x_compared']


# ---- 3. the LARGE build's capacity guard ----
def test_large_build_capacity_overflow_fails_loudly():
    """N = 100 with its eight contact times per foot 0.2 s apart needs n_u = 288 > 240 (the oracle's count): SRBM_ERR_CAPACITY and status 8,
    as the standard build reports beyond 160 (tests/test_gpu_parity.py::test_capacity_overflow_fails_loudly).  (The schedules tried on the
    oracle -- N = 40 .. 100, dt 0.02 / 0.05, 0.05 .. 0.2 s phases, up to 8 contact times per foot -- gave n_u in {120, 148, 172, 204, 232, 288,
    ...}; none in 233 .. 240.  The dense hooks cover n = 233 .. 240: tests/test_gpu_dense.py.)"""
    cfg = load_config(num_nodes=100, integrator_dt=0.02)
    nu, _, _ = first_rti_sizes(cfg, PHASE_OVERFLOW)
    assert nu == 288 and nu > host.lib(True).capacity['nu']
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, EE_NOMINAL, large=True)
    set_phases(g, PHASE_OVERFLOW)
    g.get_real_time_update(s0, 0.0, EE_NOMINAL)
    st, err = g.status()
    assert np.all(err & 16) and np.all(st == 8), (st, err)
