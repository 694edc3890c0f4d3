"""Host-only pins of tests/lp_reference.py: its rows against the oracle's restatement of the same LP on the reference configurations, and the
conditions the seeded cases of tests/test_gpu_gait_lp.py have to meet before they are worth a GPU."""
import numpy as np
import pytest

import lp_reference as R
from gpu_kit import REL_TOL
from oracle_py import OracleMPC, load_config
from srbm_loader.workloads import EE_NOMINAL


@pytest.mark.parametrize('cfgname,nsteps', [('a1_configuration', 3), ('a1_gait_opt_config', 2)])
def test_rows_give_the_oracles_lp_value_and_step(cfgname, nsteps):
    """the open-loop RTI run of test/gait_opt_playground.cpp:113-126 on the oracle alone; then GaitOptimizer::OptimizeContactTimes of the oracle
    against build_lp + solve_lp on the oracle's gradient and contact times: value to REL_TOL, step to 1e-4 on the entries whose cost
    coefficient is not ~0 (the bar of test_contact_time_lp_matches_oracle)"""
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    o = OracleMPC(cfg)
    o.set_warmstart(s0)
    o.initial_run(s0, EE_NOMINAL)
    dt = cfg['integrator_dt']
    for i in range(nsteps):
        t = i * dt
        state = o.states()[1]
        ee = np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])
        o.rti(state, t, ee)
    go = o.gait_gradient()
    assert go is not None
    nv = len(go)
    cts, kinds = zip(*[o.contact_times(e) for e in range(4)])
    assert sum(len(c) for c in cts) == nv
    step_o, _ = o.gait_optimize(t)
    ref = R.solve_lp(go, *R.build_lp(list(cts), list(kinds), t))
    assert ref['feasible'] and ref['certified'], ref
    val_o = go @ step_o[:nv]
    print('LP value [%s, %d]: exact %.9g oracle %.9g' % (cfgname, nsteps, ref['f'], val_o))
    assert abs(ref['f'] - val_o) <= REL_TOL * max(1.0, abs(val_o))
    big = np.abs(go) > 1e-3 * np.abs(go).max()
    assert np.abs(ref['x'] - step_o[:nv])[big].max() <= 1e-4


def test_a_foot_past_its_last_contact_time_has_no_next_node_rows():
    cts = [np.array([0.0, 0.3, 0.7]), np.array([0.0, 0.4])]
    kinds = [np.array([R.LO, R.TD, R.LO]), np.array([R.TD, R.LO])]
    assert R.next_node(cts[0], 0.5) == 2 and R.next_node(cts[0], 0.7) == 2 and R.next_node(cts[0], -1.0) == 1 and R.next_node(cts[0], 0.71) is None
    A_ub, b_ub, A_eq, b_eq = R.build_lp(cts, kinds, 0.2)             # foot 0: touch-down at index 1 next; foot 1: a lift-off next
    assert A_eq.shape == (4, 5) and np.array_equal(np.nonzero(R.pinned_columns(A_eq))[0], [0, 1, 3])
    assert A_ub.shape == (2 * (2 + 1) + 2 * (1 + 1) + 2 * 5, 5) and R.lane_rows([3, 2]) == 20
    assert b_ub[0] == 0.3 and b_ub[1] == 3.0 and b_ub[2] == 0.7 - 0.3 - 0.2 and b_ub[3] == 2.0 and b_ub[4] == 1.0 and b_ub[5] == 0.0
    A_ub, b_ub, A_eq, b_eq = R.build_lp(cts, kinds, 5.0)
    assert A_eq.shape == (2, 5) and b_ub[0] == 0.3 - 0.2


def test_seeded_cases_meet_their_conditions():
    """the generator of the GPU module, run on the host: at most 10 % of its draws infeasible, at least 90 % of the feasible generic-gradient
    cases at a nondegenerate vertex (they take the entrywise check), every reference certified, the cases built to be infeasible infeasible"""
    import test_gpu_gait_lp as T
    A, Bb, ix = T.cases()
    gen = A[:ix['n_generic']]
    feas = [c for c in gen if c['ref']['feasible']]
    assert len(gen) - len(feas) <= 0.1 * len(gen), len(feas)
    assert all(c['ref']['certified'] for c in feas)
    plain = [c for c in feas if c['grad_how'] == 'generic']
    assert len(plain) >= 30 and sum(c['nondegenerate'] for c in plain) >= 0.9 * len(plain)
    assert sum(not c['ref']['feasible'] for c in A if c['time_how'] == 'infeasible') == 3
    assert len(A) == T.B and len(Bb) == T.B and len(ix['scale']) == 3 * len(T.SCALES)
    for case in A + Bb:
        for kk, tt in case['table']:
            assert len(kk) <= R.KMAX and kk[0] <= R.TD and np.all(np.diff(tt) >= 0)
    # every time case puts the next contact time where it says
    for c in gen:
        nn = [R.next_node(ct, c['tnow']) for ct in c['cts']]
        if c['time_how'] == 'after':
            assert all(n is None for n in nn)
        if c['time_how'] == 'before':
            assert all(n == 1 for n in nn)
        if c['time_how'] == 'td_first':
            assert any(n == 1 and k[1] == R.TD for n, k in zip(nn, c['kinds']))
        if c['time_how'] == 'td_last':
            assert any(n == len(k) - 1 and k[-1] == R.TD for n, k in zip(nn, c['kinds']))
        if c['time_how'] == 'lift_off':
            assert any(n is not None and k[n] == R.LO for n, k in zip(nn, c['kinds']))
        if c['time_how'] == 'equal':
            assert any(c['tnow'] in ct[1:] for ct in c['cts'])
