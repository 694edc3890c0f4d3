"""What the condensing kernel leaves in the work record -- H, g, the compact dense state rows Sig / sig0 -- against a dense numpy elimination of
the full-space QP that export_qp returns for the same instance and step (the resync tests hold that QP to the oracle at 1e-12).

Reference (reference_condensed): the states are eliminated through the dynamics rows (x = S u + s), the pinned and substituted position variables
through the TD / start rows (u = Z v + u0, the dependent variable of a row is its first coefficient); H_ref = Z'(P_uu + S' P_xx S) Z,
g_ref = Z'(S'(P_xx (s + S u0) + q_x) + P_uu u0 + q_u), state rows S Z and s + S u0, all in the kernel's variable order.  On the free variables H and
g are compared; a pinned variable is an identity row of H with zero gradient, asserted exactly; Sig / sig0 are the position rows (x, y of nodes 4..N)
on the force variables of their coordinate, the rest of such a row is zero in the reference to rounding and checked by the kernel itself
(SRBM_ERR_STRUCTURE); the error bits are 0.  Every instance is compared at every step, also one whose oracle gave up (it continues on its own path).

Cases: the smallest shapes at which the condensing and the assembly can go wrong -- N = 10 (4 Config-B instances, 7 steps: n_u 120 and 92),
N = 20 (8 instances, the four cost sets of tests/cost_variants_kit.py interleaved: the diagonal and the full 12 x 12 path; 6 steps: n_u 120 and 148),
N = 50 (2 Config-D instances, 12 steps: the larger window enters at step 11), each re-synchronised to the oracle before every step, through the
fused launch and through the stand-alone kernels; N = 40 on the LARGE build (2 instances, sets B and C, 4 steps: n_u 204 and 232).  Each case
asserts that both window sizes, a substituted variable and a touch-down pin occurred.

Tolerance: the largest relative difference (max |a - ref| / max |ref| per array, instance and step) measured with the kernels as they were when the
read-out was added (the kernels since compute the same bits: scripts/dev_bitwise_ab.py), over all cases:
    H 4.55e-14 (N = 50)   g 2.57e-13 (N = 20)   Sig 3.99e-14 (N = 50)   sig0 8.56e-14 (N = 20)
and four times that is the bound (another summation order in numpy moves the last bits; the kernel's own result may not move at all)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cost_variants_kit import SETS, cost_set
from gpu_kit import status_four_classes as cls
from gpu_protocols import make_batch
from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, config_d_instance, instances

pytestmark = pytest.mark.gpu

MEASURED = dict(H=4.55e-14, g=2.57e-13, Sig=3.99e-14, sig0=8.56e-14)
BOUND = {k: 4 * v for k, v in MEASURED.items()}


def reference_condensed(A, b, P, q, N, n_eq_u):
    """the dense elimination of the module's docstring: dict(H, g, SZ [12 (N + 1)][n_u], s0 [12 (N + 1)], dep: the pinned / substituted variables)"""
    nx = 12 * (N + 1)
    n, m = P.shape[0], A.shape[0]
    nu = n - nx
    Ax, Au = A[:nx, :nx], A[:nx, nx:]
    S, s = -np.linalg.solve(Ax, Au), np.linalg.solve(Ax, b[:nx])
    assert not np.any(A[m - n_eq_u:, :nx]) and not np.any(P[:nx, nx:]) and not np.any(P[nx:, :nx])
    E, e = A[m - n_eq_u:, nx:], b[m - n_eq_u:]
    dep = [int(np.nonzero(r)[0][0]) for r in E]
    assert len(set(dep)) == len(dep)
    free = np.array([j for j in range(nu) if j not in dep], int)
    Z, u0 = np.zeros((nu, nu)), np.zeros(nu)
    Z[free, free] = 1.0
    Z[np.ix_(dep, free)] = -np.linalg.solve(E[:, dep], E[:, free])
    u0[dep] = np.linalg.solve(E[:, dep], e)
    Pxx, Puu = P[:nx, :nx], P[nx:, nx:]
    H = Z.T @ (Puu + S.T @ Pxx @ S) @ Z
    g = Z.T @ (S.T @ (Pxx @ (s + S @ u0) + q[:nx]) + Puu @ u0 + q[nx:])
    return dict(H=H, g=g, SZ=S @ Z, s0=s + S @ u0, dep=np.array(sorted(dep)), free=free)


def rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def column_map(g, b):
    """(col_ee, col_type, col_coord, col_local)[NUMAX] and fix_mask[NUMAX] of instance b (srbm_debug_get_spline_step)"""
    NU = g.NUMAX
    up = np.zeros(NU); u = np.zeros(NU); cols = np.zeros((4, NU), np.int32); fix = np.zeros(NU, np.int32)
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    g._chk(g.L.srbm_debug_get_spline_step(g.h, int(b), up.ctypes.data_as(DP), u.ctypes.data_as(DP), cols.ctypes.data_as(IP), fix.ctypes.data_as(IP)))
    return cols, fix


def compare_instance(g, b, N, where):
    """one instance after a step: the condensed arrays against the elimination of its own exported QP; returns the relative differences and what
    the step held (n_u, a substituted variable, a touch-down pin)"""
    sz = g.sizes()[b]
    A, bv, P, q = g.export_qp(b)
    ref = reference_condensed(A, bv, P, q, N, int(sz[6]) + 8)
    cd = host.condensed(g, b)
    cols, fix = column_map(g, b)
    nu = cd['nu']
    assert cd['err'] == 0 and nu == int(sz[0]) - 12 * (N + 1), (where, cd['err'], nu)
    dep, free = ref['dep'], ref['free']
    assert np.array_equal(np.nonzero(fix[:nu])[0], dep), where             # the kernel's pinned / substituted variables are the reference's
    # pinned variables: identity rows, zero gradient -- exactly
    eye = np.eye(nu)
    assert np.array_equal(cd['H'][dep], eye[dep]) and np.array_equal(cd['H'][:, dep], eye[:, dep]) and not np.any(cd['g'][dep]), where
    out = dict(H=rel(cd['H'][np.ix_(free, free)], ref['H'][np.ix_(free, free)]), g=rel(cd['g'][free], ref['g'][free]))
    # dense state rows: position c of node k on the force variables of coordinate c over the four feet, in column order
    rows = np.array([12 * k + c for k in range(4, N + 1) for c in range(2)])
    sig_ref = np.zeros_like(cd['Sig'])
    wc = 0
    for c in range(2):
        jc = np.nonzero((cols[1, :nu] == 0) & (cols[2, :nu] == c))[0]
        wc = max(wc, len(jc))
        sig_ref[c::2, :len(jc)] = ref['SZ'][rows[c::2]][:, jc]
        other = np.setdiff1d(np.arange(nu), jc)
        assert np.abs(ref['SZ'][rows[c::2]][:, other]).max() <= 1e-10 * np.abs(ref['SZ']).max(), where
    out['Sig'] = rel(cd['Sig'][:, :wc], sig_ref[:, :wc])
    out['sig0'] = rel(cd['sig0'], ref['s0'][rows])
    print('%s: n_u %d  H %.2e  g %.2e  Sig %.2e  sig0 %.2e' % (where, nu, out['H'], out['g'], out['Sig'], out['sig0']))
    for k in BOUND:
        assert out[k] <= BOUND[k], (where, k, out[k], BOUND[k])
    return out, dict(nu=nu, sub=bool(np.any(fix[:nu] == 2)), td=int(sz[6]) > 0)


def run_case(cfg, make_inst, B, steps, fused, large=None, costs=None):
    """the re-synchronised protocol of gpu_protocols.resync_protocol, reduced to what this module compares: before every step the device is given
    the oracle's trajectory (its own where the oracle's solver gave up), steps through the fused launch (srbm_rti_advance(i, 1)) or the
    stand-alone kernels (srbm_get_real_time_update), and every instance is compared"""
    N, dt = cfg['num_nodes'], cfg['integrator_dt']
    states, ees = instances(cfg, make_inst, B)
    g, oracles = make_batch(cfg, states, ees, True, large, costs)
    if fused:
        g.set_solver_step_rule(g.solver_step_rule()[0], host.FAST_START_MU)
    pool = ThreadPoolExecutor(8)
    list(pool.map(lambda b: oracles[b].initial_run(states[b], ees[b].reshape(4, 3)), range(B)))
    g.create_initial_run(states, ees.reshape(B, 12))
    alive = np.ones(B, bool)
    worst, seen = dict.fromkeys(BOUND, 0.0), []
    for i in range(steps):
        t = i * dt
        own = g.get_trajectory()
        g.set_warm_start_trajectory((host.Trajectory * B)(*[oracles[b].trajectory_record(host) if alive[b] else own[b] for b in range(B)]))
        own_states = g.trajectory_states()
        _, own_ee, _ = g.eval_trajectory(t)
        st_in = np.array([(o.states()[1] if (i > 0 or fused) else states[b]) if alive[b] else own_states[b, 1] for b, o in enumerate(oracles)])
        ee_in = np.array([[[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)] if alive[b] else own_ee[b]
                          for b, o in enumerate(oracles)]).reshape(B, 12)
        if fused:
            g.rti_advance(i, 1); g.synchronize()
        else:
            g.get_real_time_update(st_in, t, ee_in)
        sos = list(pool.map(lambda b: oracles[b].rti(st_in[b], t, ee_in[b].reshape(4, 3)) if alive[b] else 8, range(B)))
        for b in range(B):
            out, held = compare_instance(g, b, N, 'N %d %s step %d instance %d' % (N, 'fused' if fused else 'stand-alone', i, b))
            seen.append(held)
            for k in worst:
                worst[k] = max(worst[k], out[k])
            if cls(sos[b]) in ('maxiter', 'other'):
                alive[b] = False
    g.close()
    print('N %d %s: worst relative differences %s' % (N, 'fused' if fused else 'stand-alone', worst))
    return seen


def assert_occurred(seen, sizes):
    assert {h['nu'] for h in seen} == set(sizes), sorted({h['nu'] for h in seen})       # both window sizes of the schedule
    assert any(h['sub'] for h in seen) and any(h['td'] for h in seen)                   # a substituted variable, a touch-down pin


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'stand_alone'])
def test_n10_config_b(fused):
    cfg = load_config(num_nodes=10)
    assert_occurred(run_case(cfg, config_b_instance, 4, 7, fused), (120, 92))


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'stand_alone'])
def test_n20_four_cost_sets_interleaved(fused):
    """sets A (diagonal path) and B, C, D (full 12 x 12 path) side by side in one batch"""
    cfg = load_config()
    costs = [cost_set(cfg, SETS[b % 4]) for b in range(8)]
    assert_occurred(run_case(cfg, config_b_instance, 8, 6, fused, costs=costs), (120, 148))


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'stand_alone'])
def test_n50_config_d(fused):
    cfg = load_config('a1_config_distr_rejection')
    assert cfg['num_nodes'] == 50
    assert_occurred(run_case(cfg, config_d_instance, 2, 12, fused), (120, 148))


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'stand_alone'])
def test_n40_large_build_sets_b_and_c(fused):
    cfg = load_config(num_nodes=40)
    seen = run_case(cfg, config_b_instance, 2, 4, fused, large=True, costs=[cost_set(cfg, 'B'), cost_set(cfg, 'C')])
    assert max(h['nu'] for h in seen) > 160                                             # beyond the standard build's capacity
