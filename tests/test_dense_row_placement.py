"""Where the IPM puts the compact dense state rows (csrc/srbm_k3_lds.hiph: k3_sig_placement, the arithmetic k3_make_smem decides with): in LDS --
the tail of the packed-matrix window and the space behind the LDS map -- or, when they do not fit, read from W.Sig in L2 in every pass.  Both
libraries answer through srbm_debug_dense_row_placement on a machine without a GPU.  The sizes of each case come from the CPU oracle (n_u = n -
12 (N + 1), wc = n_force / 3), so the pins hold the schedules the end-to-end tests run (tests/test_gpu_dense_rows.py) to the branch they exist
to reach."""
import pytest

from oracle_py import first_rti_sizes, load_config
from srbm_loader import host


# (build, config, N, dt, phases) -> (n_u, wc) of the first step, (rows in the window's tail, rows behind the map, all in LDS)
CASES = [
    (False, 'a1_configuration', 20, 0.05, None, (120, 32), (34, 0, True)),               # Config B
    (False, 'a1_config_distr_rejection', 50, 0.02, None, (120, 32), (94, 0, True)),      # Config D
    (False, 'a1_config_distr_rejection', 50, 0.02, 0.2, (148, 40), (46, 0, False)),      # Config D's horizon, 0.2 s phases (the gait LP's MIN_TIME): L2
    (False, 'a1_config_distr_rejection', 50, 0.02, 0.22, (148, 40), (46, 0, False)),     # ... 0.22 s phases (tests/test_gpu_dense_rows.py: n_u 148 for five steps)
    (True, 'a1_configuration', 40, 0.05, None, (204, 56), (0, 74, True)),                # Config E (N = 40)
    (True, 'a1_configuration', 75, 0.02, None, (172, 48), (0, 144, True)),               # N = 75: LDS
    (True, 'a1_configuration', 100, 0.02, None, (204, 56), (0, 136, False)),             # N = 100, the reference's limit: L2
]


@pytest.mark.parametrize('large,name,N,dt,phase,sizes,placement', CASES)
def test_dense_row_placement_of_the_schedules_the_suite_runs(large, name, N, dt, phase, sizes, placement):
    nu, wc, _ = first_rti_sizes(load_config(name, num_nodes=N, integrator_dt=dt), phase)
    assert (nu, wc) == sizes
    assert host.dense_row_placement(N, nu, wc, large) == placement


def test_dense_row_placement_at_the_capacity_limits():
    # standard build: the window's tail shrinks with n_u; behind the map there is room for 21 doubles at N = 50, none for a row
    assert host.dense_row_placement(50, 160, 40) == (0, 0, False)
    assert host.dense_row_placement(50, 120, 40) == (94, 0, True)
    assert host.dense_row_placement(20, 160, 48) == (0, 29, False)        # a full window at N = 20: 29 of 34 rows behind the map
    # LARGE build: no window tail (the matrix is in global memory), everything behind the map
    assert host.dense_row_placement(40, 232, 64, True) == (0, 74, True)
    assert host.dense_row_placement(100, 240, 64, True) == (0, 119, False)
    with pytest.raises(ValueError):
        host.dense_row_placement(100, 120, 32)            # beyond the standard build's horizon
    with pytest.raises(ValueError):
        host.dense_row_placement(40, 241, 64, True)       # beyond the LARGE build's n_u
