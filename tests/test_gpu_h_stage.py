"""The two things every IPM iteration takes for granted (bilevel-gait-gen_amd/csrc/srbm_k3_normal.hiph: k3_load_h_o; srbm_k3_lds.hiph: k3_make_smem,
k3_publish_smem), through the hook srbm_debug_h_stage of csrc/srbm_dense_hooks.hiph, which runs the routines the IPM runs:

1. The staging of H.  The standard build copies the packed Hessian into the LDS by LDS-DMA in 1 KiB pieces of 16-byte units; the LARGE build copies it
   through registers into the work record.  Either way exactly np = n (n + 1) / 2 doubles arrive, bit for bit, and the doubles behind them -- in a
   solve the compact dense rows begin there -- keep what they held.  Compared as uint64: the payload is random bit patterns with NaNs (quiet and
   signalling, with payloads), +-Inf, denormals and -0 among them, and it holds them at its first and last elements, the ones the tail handling moves.
2. The LDS map an out-of-line phase reads back after the prologue of the solve published it: the placement of the compact dense rows is the one
   k3_sig_placement gives (srbm_debug_dense_row_placement; tests/test_dense_row_placement.py pins that on the CPU), on both sides of the point where
   the rows stop fitting the LDS."""
import ctypes as C

import numpy as np
import pytest

from srbm_loader import host

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)          # DBG_H_STAGE_SENTINEL
GUARD = 64
SPECIALS = np.array([0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8DEADBEEF0000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x8000000000000000, 0x000FFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF], np.uint64)
# np odd and even, less than one 16-byte unit, less than one wave's piece | ... | np straddles 1024 doubles: one piece per wave | ... | the two sizes
# the workload alternates between | the last row ends at SRBM_HPACK
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 44, 45, 63, 64, 65, 120, 148, 159, 160]
dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))


def payload(n, count):
    npk = n * (n + 1) // 2
    rng = np.random.default_rng(1000 + n)
    H = rng.integers(0, 2 ** 64, size=(count, npk), dtype=np.uint64)
    where = np.unique(np.concatenate([[0, npk - 1, npk - 2, npk // 2], rng.integers(0, npk, size=min(npk, 24))]) % npk)
    for b in range(count):
        H[b, where] = SPECIALS[(np.arange(len(where)) + n + b) % len(SPECIALS)]
    assert not (H == SENTINEL).any()
    return H


def stage(lib, n, H, guard, N=0, wc=0, with_map=False):
    count, npk = H.shape
    out = np.zeros((count, npk + guard), np.uint64)
    m = np.full((count, 5), -1, np.int32)
    rc = lib.srbm_debug_h_stage(n, count, dp(H), dp(out), guard, N, wc, m.ctypes.data_as(C.POINTER(C.c_int)) if with_map else None)
    assert rc == 0, lib.srbm_last_error().decode()
    return out, m


@pytest.mark.parametrize('large', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_staging_moves_exactly_the_packed_matrix_bit_for_bit(large, n):
    H = payload(n, 2)
    npk = H.shape[1]
    out, _ = stage(host.lib(large), n, H, GUARD)
    bad = np.argwhere(out[:, :npk] != H)
    assert len(bad) == 0, 'n %d: matrix differs at (workgroup, element) %s of %d' % (n, bad[:8].tolist(), npk)
    touched = np.argwhere(out[:, npk:] != SENTINEL)
    assert len(touched) == 0, 'n %d: doubles behind the matrix written at (workgroup, offset) %s' % (n, touched[:8].tolist())


# (build, N, n_u, wc): the first steps of Config B and D, Config D's horizon at n_u 148 (rows in L2), Config B's at 148, the capacity limits of
# tests/test_dense_row_placement.py; the LARGE build's schedules on both sides of its limit
MAPS = [(False, 20, 120, 32), (False, 50, 120, 32), (False, 50, 148, 40), (False, 20, 148, 40), (False, 50, 160, 40), (False, 50, 120, 40),
        (False, 20, 160, 48), (True, 40, 204, 56), (True, 75, 172, 48), (True, 100, 204, 56)]


@pytest.mark.parametrize('large,N,nu,wc', MAPS)
def test_map_read_back_by_a_phase_is_the_placement_rule(large, N, nu, wc):
    in_tail, in_extra, all_lds = host.dense_row_placement(N, nu, wc, large)
    assert all_lds == (in_tail + in_extra == 2 * (N - 3))
    H = payload(nu, 1)
    out, m = stage(host.lib(large), nu, H, GUARD, N, wc, True)
    assert m[0, :4].tolist() == [wc, in_tail, int(all_lds), 0 if large else nu * (nu + 1) // 2]
    assert (out[0, :H.shape[1]] == H[0]).all() and (out[0, H.shape[1]:] == SENTINEL).all()       # (the slots of the map are not in the matrix window)


def test_both_sides_of_the_fit_are_among_the_cases():
    fits = {(large, host.dense_row_placement(N, nu, wc, large)[2]) for large, N, nu, wc in MAPS}
    assert fits == {(False, True), (False, False), (True, True), (True, False)}
