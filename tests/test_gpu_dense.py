"""GPU unit tests of the dense fp64 building blocks of the IPM kernel (bilevel-gait-gen_amd/csrc/srbm_dense.hiph, srbm_k3_normal.hiph, srbm_k3_rows.hiph) against
numpy, in both builds: the standard one (packed matrix in LDS, n <= 160) and the LARGE one (packed matrix in global memory, n <= 240,
DN_MAXT = DN_SLOTS = 15), through the hooks of csrc/srbm_dense_hooks.hiph.

Tolerances: the Cholesky's backward error |L L' - M| <= 1e-13 |M| (fp64 Cholesky is backward stable; the entries of L themselves are compared to
1e-9 relative on well-conditioned inputs only).  The inverse factor and the solve are held to normwise backward errors, eps = 2^-53, C_BWD = 4:
    |X L - I|_inf <= C_BWD n eps |X|_inf |L|_inf            |M x - b|_inf <= C_BWD n eps (|M|_inf |x|_inf + |b|_inf)
(residuals in long double; a backward-stable fp64 computation lands near n eps).  The mat-vecs entry by entry: |y_i - (H x)_i| <= C_MV n eps
(|H| |x|)_i, C_MV = 2, against a long-double product.  The doubles after the packed matrix, which the helpers may read but must not use, are set
to a fill value: every output must be bitwise the same for a fill of 0, of finite random values, of +-Inf and of NaN."""
import ctypes as C
import numpy as np
import pytest

from srbm_loader import host

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
C_BWD = 4.0
C_MV = 2.0
LARGE_ONLY = [161, 175, 176, 177, 192, 204, 208, 224, 232, 233, 239, 240]      # n_u beyond the standard build (DN_MAXT 11 .. 15)
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def inorm(A):
    A = np.atleast_2d(A)
    return np.abs(A).sum(axis=1).max()


def pack(M):
    n = M.shape[0]
    return np.concatenate([M[i, :i + 1] for i in range(n)])


def unpack(p, n):
    L = np.zeros((n, n))
    k = 0
    for i in range(n):
        L[i, :i + 1] = p[k:k + i + 1]; k += i + 1
    return L


def device_cholesky(mats, large=False, fill=0.0, raw=False):
    lib = host.lib(large)
    n = mats[0].shape[0]
    inp = np.ascontiguousarray(np.stack([pack(M) for M in mats]))
    out = np.zeros_like(inp); nreg = np.zeros(len(mats), np.int32)
    rc = lib.srbm_debug_cholesky(n, len(mats), dp(inp), dp(out), ip(nreg), C.c_double(fill))
    assert rc == 0, lib.srbm_last_error().decode()
    device_cholesky.ticks = (nreg >> 8) * 16      # diagnostic: s_memtime ticks of load + factorisation
    if raw:
        return out, nreg & 0xff
    return [unpack(o, n) for o in out], nreg & 0xff


def device_solve(mats, rhs, large=False, fill=0.0):
    lib = host.lib(large)
    n = mats[0].shape[0]
    inp = np.ascontiguousarray(np.stack([pack(M) for M in mats])); r = np.ascontiguousarray(np.stack(rhs))
    x = np.zeros_like(r); X = np.zeros_like(inp); ticks = np.zeros(2 * len(mats), np.int32)
    rc = lib.srbm_debug_solve(n, len(mats), dp(inp), dp(r), dp(x), dp(X), ip(ticks), C.c_double(fill))
    assert rc == 0, lib.srbm_last_error().decode()
    device_solve.ticks = ticks.reshape(-1, 2)
    device_solve.raw = X
    return x, [unpack(v, n) for v in X]


def device_solve_mapped(mats, rhs, free, large=False, fill=0.0):
    lib = host.lib(large)
    n = mats[0].shape[0]
    inp = np.ascontiguousarray(np.stack([pack(M) for M in mats])); r = np.ascontiguousarray(np.stack(rhs))
    x = np.zeros_like(r); nreg = np.zeros(len(mats), np.int32)
    free = np.ascontiguousarray(free, np.int32)
    rc = lib.srbm_debug_solve_mapped(n, len(free), ip(free), len(mats), dp(inp), dp(r), dp(x), ip(nreg), C.c_double(fill))
    assert rc == 0, lib.srbm_last_error().decode()
    return x, nreg


def solve_backward_error(M, x, b):
    """|M x - b|_inf / (n eps (|M|_inf |x|_inf + |b|_inf)), the residual in long double"""
    n = M.shape[0]
    r = M.astype(np.longdouble) @ x.astype(np.longdouble) - b.astype(np.longdouble)
    return float(np.abs(r).max()) / (n * EPS * (inorm(M) * np.abs(x).max() + np.abs(b).max()))


def inverse_backward_error(X, L):
    """|X L - I|_inf / (n eps |X|_inf |L|_inf), the product in long double"""
    n = L.shape[0]
    R = X.astype(np.longdouble) @ L.astype(np.longdouble) - np.eye(n, dtype=np.longdouble)
    return float(np.abs(R).sum(axis=1).max()) / (n * EPS * inorm(X) * inorm(L))


CHOL_SIZES = [1, 3, 4, 15, 16, 17, 63, 64, 118, 120, 157, 160]


def check_cholesky(n, large):
    rng = np.random.default_rng(n)
    mats = []
    for _ in range(3):
        A = rng.standard_normal((n, n + 5))
        mats.append(A @ A.T + 0.1 * np.eye(n))
    Ls, nreg = device_cholesky(mats, large)
    assert np.all(nreg == 0)
    for M, L in zip(mats, Ls):
        assert np.abs(np.triu(L, 1)).max() == 0
        assert np.abs(L @ L.T - M).max() <= 1e-13 * np.abs(M).max()
        Lr = np.linalg.cholesky(M)
        assert np.abs(L - Lr).max() <= 1e-9 * np.abs(Lr).max()


@pytest.mark.parametrize('n', CHOL_SIZES)
def test_mfma_cholesky_matches_numpy(n):
    check_cholesky(n, False)


@pytest.mark.parametrize('n', CHOL_SIZES + LARGE_ONLY)
def test_mfma_cholesky_matches_numpy_large_build(n):
    check_cholesky(n, True)


def test_mfma_cholesky_barrier_weighted_matrix():
    """the shape the IPM produces: H with curvature 1e-3 plus G' W G with weights spread over 14 decades"""
    rng = np.random.default_rng(7)
    n, m = 120, 752
    G = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.05)
    w = 10.0 ** rng.uniform(-4, 10, m)
    M = 1e-3 * np.eye(n) + G.T @ (w[:, None] * G)
    (L,), nreg = device_cholesky([M])
    assert nreg[0] == 0
    assert np.abs(L @ L.T - M).max() <= 1e-13 * np.abs(M).max()


@pytest.mark.parametrize('n,m', [(120, 752), (232, 1432)])
def test_mfma_cholesky_barrier_weighted_matrix_large_build(n, m):
    """... in the LARGE build, at Config B's shape and at the N = 40 shape (n_u 232, ~1400 inequality rows)"""
    rng = np.random.default_rng(7 + n)
    G = rng.standard_normal((m, n)) * (rng.random((m, n)) < 0.05)
    w = 10.0 ** rng.uniform(-4, 10, m)
    M = 1e-3 * np.eye(n) + G.T @ (w[:, None] * G)
    (L,), nreg = device_cholesky([M], True)
    assert nreg[0] == 0
    assert np.abs(L @ L.T - M).max() <= 1e-13 * np.abs(M).max()


def test_mfma_cholesky_reports_indefinite_input():
    n = 40
    M = np.eye(n); M[17, 17] = -1.0
    (L,), nreg = device_cholesky([M])
    assert nreg[0] == 1


def test_mfma_cholesky_reports_indefinite_input_large_build():
    n = 233
    M = np.eye(n); M[217, 217] = -1.0
    (L,), nreg = device_cholesky([M], True)
    assert nreg[0] == 1


SOLVE_SIZES = [1, 5, 16, 17, 33, 64, 100, 120, 128, 129, 144, 157, 160]


def check_solve(n, large):
    """X = L^-1 by MFMA tile products, then x = X'(X b): against numpy, and normwise backward errors"""
    rng = np.random.default_rng(100 + n)
    mats, rhs = [], []
    for _ in range(2):
        A = rng.standard_normal((n, n + 3))
        mats.append(A @ A.T + 0.5 * np.eye(n)); rhs.append(rng.standard_normal(n))
    x, Xs = device_solve(mats, rhs, large)
    worst = [0.0, 0.0]
    for M, b, xv, X in zip(mats, rhs, x, Xs):
        L = np.linalg.cholesky(M)
        assert np.abs(X @ L - np.eye(n)).max() <= 1e-10 * np.linalg.cond(L)
        xr = np.linalg.solve(M, b)
        assert np.abs(xv - xr).max() <= 1e-9 * max(1.0, np.abs(xr).max()) * np.linalg.cond(M) ** 0.5
        worst = [max(worst[0], inverse_backward_error(X, L)), max(worst[1], solve_backward_error(M, xv, b))]
    print('n = %d: backward errors in units of n eps: inverse factor %.3f, solve %.3f' % (n, worst[0], worst[1]))
    assert worst[0] <= C_BWD and worst[1] <= C_BWD, worst


@pytest.mark.parametrize('n', SOLVE_SIZES)
def test_explicit_factor_inverse_and_solve(n):
    check_solve(n, False)


@pytest.mark.parametrize('n', SOLVE_SIZES + LARGE_ONLY)
def test_explicit_factor_inverse_and_solve_large_build(n):
    check_solve(n, True)


def mapped_problem(n, nfix, count=3):
    rng = np.random.default_rng(7000 + 31 * n + nfix)
    fixed = np.sort(rng.choice(n, nfix, replace=False))
    free = np.setdiff1d(np.arange(n), fixed).astype(np.int32)
    mats, rhs = [], []
    for _ in range(count):
        G = rng.standard_normal((2 * n, n)); w = 10.0 ** rng.uniform(-3, 8, 2 * n)
        M = 1e-2 * np.eye(n) + G.T @ (w[:, None] * G)
        M[fixed, :] = 0; M[:, fixed] = 0; M[fixed, fixed] = 1.0
        b = rng.standard_normal(n); b[fixed] = rng.standard_normal(nfix) * (rng.random(nfix) < 0.5)      # the IPM's are zero there; any value must survive
        mats.append(M); rhs.append(b)
    return fixed, free, mats, rhs


def check_mapped(n, nfix, large):
    lib = host.lib(large)
    fixed, free, mats, rhs = mapped_problem(n, nfix)
    x, nreg = device_solve_mapped(mats, rhs, free, large)
    assert np.all(nreg == 0)
    worst = 0.0
    for M, b, xv in zip(mats, rhs, x):
        xr = np.linalg.solve(M, b)
        assert np.array_equal(xv[fixed], b[fixed])
        Mf = M[np.ix_(free, free)]
        assert np.abs(xv - xr).max() <= 1e-9 * max(1.0, np.abs(xr).max()) * np.linalg.cond(Mf) ** 0.5
        worst = max(worst, solve_backward_error(M, xv, b))
    print('n = %d, %d pinned: backward error of the mapped solve in units of n eps %.3f' % (n, nfix, worst))
    assert worst <= C_BWD, worst
    # a map that is not increasing is refused
    bad = free.copy(); bad[[0, 1]] = bad[[1, 0]]
    inp = np.ascontiguousarray(np.stack([pack(M) for M in mats])); r = np.ascontiguousarray(np.stack(rhs)); nr = np.zeros(1, np.int32)
    if len(bad) > 1: assert lib.srbm_debug_solve_mapped(n, len(bad), ip(bad), 1, dp(inp), dp(r), dp(x), ip(nr), C.c_double(0.0)) != 0


@pytest.mark.parametrize('n,nfix', [(20, 3), (120, 8), (120, 12), (120, 16), (137, 9), (148, 12), (160, 8), (160, 1), (33, 30)])
def test_dense_phase_on_a_subset_of_the_columns(n, nfix):
    """the IPM's dense phase leaves the pinned / substituted position variables (identity rows of the normal matrix) out: tiles loaded
    through an increasing column map, factor and inverse of the free block, solves that gather and scatter through the map.  Against a
    numpy solve of the FULL system with the identity rows in place; entries outside the map keep the right-hand side's value."""
    check_mapped(n, nfix, False)


@pytest.mark.parametrize('n,nfix', [(20, 3), (120, 8), (148, 12), (160, 8), (33, 30), (204, 8), (204, 16), (232, 12), (232, 16), (240, 8), (240, 13)])
def test_dense_phase_on_a_subset_of_the_columns_large_build(n, nfix):
    check_mapped(n, nfix, True)


FILLS = [0.0, 'random', np.inf, -np.inf, np.nan]


@pytest.mark.parametrize('large,n', [(False, 17), (False, 119), (False, 157), (True, 17), (True, 119), (True, 157), (True, 177), (True, 233)])
def test_outputs_do_not_depend_on_the_doubles_after_the_matrix(large, n):
    """dn_raw_below (the one-block-ahead operands of dn_trtri_column) and chol_invert_diag_blocks read up to 15 doubles past the packed matrix
    when n is not a multiple of 16 -- the LDS window's tail in the standard build, the pad after the slice in the LARGE build.  Those values
    must not reach any output: Cholesky, inverse factor, solve and mapped solve are bitwise the same for every fill."""
    rng = np.random.default_rng(900 + n)
    A = rng.standard_normal((n, n + 4))
    mats = [A @ A.T + 0.3 * np.eye(n)]
    rhs = [rng.standard_normal(n)]
    # the mapped solve through the identity map (nc = n): its factor then ends where the packed matrix ends, and the doubles read past it are the
    # fill (with pinned columns the factor of the nc(nc + 1) / 2 mapped entries is followed by stale entries of the n x n matrix instead)
    fixed, free, mmats, mrhs = mapped_problem(n, 0, count=1)
    assert len(free) == n
    ref = None
    for f in FILLS:
        fills = [rng.uniform(-1e300, 1e300), rng.standard_normal() * 1e-300, rng.standard_normal()] if f == 'random' else [f]
        for fv in fills:
            L, nreg = device_cholesky(mats, large, fv, raw=True)
            x, _ = device_solve(mats, rhs, large, fv)
            xm, nm = device_solve_mapped(mmats, mrhs, free, large, fv)
            out = (L.tobytes(), nreg.tobytes(), x.tobytes(), device_solve.raw.tobytes(), xm.tobytes(), nm.tobytes())
            assert np.all(np.isfinite(L)) and np.all(np.isfinite(x)) and np.all(np.isfinite(xm)), fv
            if ref is None:
                ref = out
            else:
                names = ['cholesky', 'pivot count', 'solve', 'inverse factor', 'mapped solve', 'mapped pivot count']
                assert out == ref, (fv, [nm_ for nm_, a, b in zip(names, out, ref) if a != b])


MATVEC_SIZES = [1, 7, 8, 9, 63, 64, 65, 120, 160]


def check_matvec(entry, n, large):
    lib = host.lib(large)
    rng = np.random.default_rng(300 + n)
    mats, xs = [], []
    for _ in range(3):
        H = rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-3, 3, (n, n))
        mats.append(H + H.T); xs.append(rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n))
    inp = np.ascontiguousarray(np.stack([pack(H) for H in mats])); xv = np.ascontiguousarray(np.stack(xs)); y = np.zeros_like(xv)
    rc = getattr(lib, entry)(n, len(mats), dp(inp), dp(xv), dp(y))
    assert rc == 0, lib.srbm_last_error().decode()
    worst = 0.0
    for H, x, yv in zip(mats, xs, y):
        yr = H.astype(np.longdouble) @ x.astype(np.longdouble)
        bound = C_MV * n * EPS * (np.abs(H) @ np.abs(x))
        err = np.abs(yv.astype(np.longdouble) - yr).astype(float)
        assert np.all(err <= bound), (entry, n, np.nonzero(err > bound)[0][:8])
        worst = max(worst, float((err / np.maximum(bound / C_MV, 1e-300)).max()))
    print('%s n = %d: worst entry error in units of n eps (|H||x|)_i: %.3f' % (entry, n, worst))


@pytest.mark.parametrize('large,n', [(False, n) for n in MATVEC_SIZES] + [(True, n) for n in MATVEC_SIZES + [200, 240]])
def test_sym_matvec_of_the_dual_residual(large, n):
    """dn_sym_matvec (H u of the dual residual) with H where the IPM keeps its normal matrix in each build"""
    check_matvec('srbm_debug_sym_matvec', n, large)


@pytest.mark.parametrize('large,n', [(False, n) for n in MATVEC_SIZES] + [(True, n) for n in MATVEC_SIZES + [200, 240]])
def test_hmatvec_packed_of_the_requalify_step_and_the_refinement(large, n):
    """hmatvec_packed (H u, H du of the requalify step and the refinement) with H in global memory as SrbmWork::H"""
    check_matvec('srbm_debug_hmatvec', n, large)
