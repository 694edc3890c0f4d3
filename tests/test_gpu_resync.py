"""Full-batch, entry-wise GPU parity with the linearisation point RE-SYNCHRONISED at every step.

Both sides of an SQP real-time iteration relinearise around their own previous solution, so a 1e-7 difference after one
solve grows along the flat directions of the weakly convex QP.  Here the oracle's trajectory is
installed on the device before every step through the reference's own entry, MPC::SetWarmStartTrajectory
(/root/reference/mpc/mpc.cpp:110-119 = srbm_set_warm_start_trajectory), so that EVERY step of EVERY instance is a
comparison on identical inputs: integer artefacts and knot times bit-exact, the assembled QP (A, b, P, q in the
reference's layout) <= 1e-12 with an identical sparsity pattern, primal / dual / trajectory <= 1e-4 relative
(BASELINE.json north_star), Armijo step equal.  The 20 steps of the Config-B protocol include windows with 148 spline
variables and steps with touch-down position rows (n_td > 0).
"""
import numpy as np
import pytest

from gpu_kit import REL_TOL
from gpu_protocols import make_batch, resync_protocol
from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, config_c_instance, config_d_instance, instances

pytestmark = pytest.mark.gpu


def test_config_b_all_256_instances_entrywise_over_20_steps():
    """the full protocol at the REFERENCE'S criterion (a new batch: srbm_set_solver_step_rule(0, 0)), host-driven (srbm_get_real_time_update): all 256
    instances x 20 steps with the strict dual bounds -- dual objective to 1e-6 of its value, stationarity 1e-7.  The bench mode has the same
    protocol through the fused launch below; the step rule on the host-driven path is covered by the Config-C / Config-D runs"""
    cfg = load_config()
    B = 256
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=20, min_alive=255, step_rule=False)       # (one instance leaves at step 2: the ORACLE reports MaxIterations there)
    nx = 21 * 12
    assert {nx + 120, nx + 148} <= r['sizes'], r['sizes']         # both window sizes were compared
    assert r['td_steps'] > 0                                      # ... and steps with touch-down position rows
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['z'] < REL_TOL and r['worst']['dual_obj'] <= 1e-6
    print('resync parity at the reference criterion, 256 x 20: alive', r['alive'], 'worst', r['worst'], 'exact status matches %d / %d' % (r['exact_status'], r['total']),
          'duals compared entry-wise (unique multipliers) in %d solves, on the row space (A\'z) in %d' % (r['z_unique'], r['duals_compared_on_row_space']), 'certified minimisers: %d' % r['certified'],
          'oracle gave up on %d solves, device certified there: %d' % (r['oracle_gave_up'], r['device_certified_where_oracle_gave_up']), 'device SolvedInacc at', r['inacc_where'])
    assert r['certified'] >= 40


def test_config_b_all_256_through_the_fused_launch_with_lower_start_attempts():
    """bench.py's `step_rule_mode`: all 256 Config-B instances over 20 steps through srbm_rti_advance(i, 1) with tol_step 1e-5 and
    start_mu 0.1 -- every solve begins with the lower-start attempt, ends by the step rule or is repeated from the standard start -- entry-wise
    against the oracle (Clarabel restatement at gap 1e-15) on identical QPs, same bounds as the host-pointer protocol above.  The headline mode,
    (0, 0.1), has the same protocol below (test_config_b_reference_criterion_with_lower_start_through_the_fused_launch)"""
    cfg = load_config()
    B = 256
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=20, min_alive=253, fused=True)      # (the ORACLE gives up on up to three instances along this protocol)
    nx = 21 * 12
    assert {nx + 120, nx + 148} <= r['sizes'], r['sizes']
    assert r['td_steps'] > 0
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['z'] < REL_TOL and r['worst']['states'] < REL_TOL
    c = r['counters']
    print('resync parity THROUGH THE FUSED LAUNCH, 256 x 20, tol_step 1e-5 / start_mu 0.1: alive', r['alive'], 'worst', r['worst'],
          'solves %d, ended by the step rule %d, began with an attempt %d, attempts repeated %d' % (c['solves'], c['step_rule'], c['low_tried'], c['low_failed']),
          'certified minimisers: %d' % r['certified'], 'duals on the row space in %d solves' % r['duals_compared_on_row_space'],
          'oracle gave up on %d solves, device certified there: %d' % (r['oracle_gave_up'], r['device_certified_where_oracle_gave_up']), 'device SolvedInacc at', r['inacc_where'])
    assert c['low_tried'] == c['solves'] and c['step_rule'] >= 0.9 * c['solves']
    assert r['certified'] >= 40


@pytest.mark.parametrize('tol_step', [1e-5, 0.0], ids=['step_rule', 'lower_start'])
def test_config_d_share_through_the_fused_launch_with_lower_start_attempts(tol_step):
    """... the Config-D share (N = 50, dt = 0.02, pushed initial momenta; the 3-rows-per-thread instance of the kernel): 64 instances x 12 steps in
    both modes bench.py runs on Config D -- (1e-5, 0.1), and the headline (0, 0.1) with the strict dual bounds of the reference's criterion.
    Which window sizes occur is decided by the oracle alone (its side of the protocol does not depend on the device): for these 64 instances
    nx + 120 spline variables at steps 0-10, nx + 148 from step 11 on (a knot enters the window), touch-down rows from step 4 on, and no give-up
    of the oracle's solver within the 12 steps.  The QPs and duals are compared at the even steps and at step 11, where the larger window first appears."""
    cfg = load_config('a1_config_distr_rejection')
    B = 64
    states, ees = instances(cfg, config_d_instance, B)
    strict = tol_step == 0.0
    r = resync_protocol(cfg, states, ees, steps=12, qp_every=2, qp_extra=(11,), fused=True, step_rule=not strict, start_mu=host.FAST_START_MU)
    nx = 51 * 12
    assert r['sizes'] == {nx + 120, nx + 148}, r['sizes']        # both window sizes were compared
    assert r['td_steps'] > 0                                      # ... and steps with touch-down position rows
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['states'] < REL_TOL
    c = r['counters']
    print('resync parity through the fused launch, config D 64 x 12, mode (%g, %g): alive' % (tol_step, host.FAST_START_MU), r['alive'], 'worst', r['worst'], c,
          'device SolvedInacc at', r['inacc_where'], 'duals on the row space in %d solves' % r['duals_compared_on_row_space'])
    assert c['low_tried'] == c['solves']
    if strict:
        assert r['worst']['z'] < REL_TOL and r['worst']['dual_obj'] <= 1e-6 and c['step_rule'] == 0, (r['worst'], c)


def test_n40_share_through_the_fused_launch_with_lower_start_attempts():
    """... and the N = 40 share (Config E, LARGE-capacity build: normal matrix in L2, up to 232 spline variables): 8 instances x 5 steps"""
    cfg = load_config(num_nodes=40)
    B = 8
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=5, qp_every=2, fused=True, large=True)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    assert max(r['sizes']) - 41 * 12 > 160                   # beyond the standard build's capacity
    print('resync parity through the fused launch, N = 40 (LARGE build) 8 x 5: alive', r['alive'], 'worst', r['worst'], r['counters'])


def test_config_b_reference_criterion_with_lower_start_through_the_fused_launch():
    """srbm_set_solver_step_rule(0, 0.1) -- THE MODE OF bench.py's HEADLINE (`lower_start`): every solve ENDS by the reference's gap criterion, the
    fused launch first attempts it from the linearisation point.  All 256 Config-B instances x 20 steps, the protocol and coverage of the other
    256 x 20 runs (both window sizes, touch-down rows, certified minimisers) with the strict dual bounds of the (0, 0) run -- dual objective to
    1e-6 of its value, stationarity 1e-7 --, every solve began with an attempt.  The oracle's own solver gives up on two of these instances
    (98 and 115, MaxIterations at step 2: its side of the protocol does not depend on the device)."""
    cfg = load_config()
    B = 256
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=20, step_rule=False, fused=True, start_mu=host.FAST_START_MU, min_alive=B - 2)
    c = r['counters']
    print('resync parity, reference criterion + lower start through the fused launch, 256 x 20: alive', r['alive'], 'worst', r['worst'], c,
          'device SolvedInacc at', r['inacc_where'], 'duals on the row space in %d solves' % r['duals_compared_on_row_space'], 'certified minimisers: %d' % r['certified'],
          'oracle gave up on %d solves, device certified there: %d' % (r['oracle_gave_up'], r['device_certified_where_oracle_gave_up']))
    nx = 21 * 12
    assert {nx + 120, nx + 148} <= r['sizes'], r['sizes']         # both window sizes were compared
    assert r['td_steps'] > 0                                      # ... and steps with touch-down position rows
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['z'] < REL_TOL and r['worst']['dual_obj'] <= 1e-6
    assert c['step_rule'] == 0 and c['low_tried'] == c['solves'] and c["low_failed"] <= 0.4 * c["solves"], c
    assert r['certified'] >= 40


def test_config_b_reference_criterion_through_the_fused_launch():
    """srbm_set_solver_step_rule(0, 0) THROUGH THE FUSED LAUNCH: the library default -- Clarabel's starting point, Clarabel's
    criterion, no attempt -- on the protocol the fused launch runs (its first step starts from node 1 of the cold-start trajectory), 64 instances x
    12 steps with the strict dual bounds.  Separates the fused protocol's QPs from the lower-start attempt: a solve the device cannot finish HERE is
    the protocol's, not the attempt's."""
    cfg = load_config()
    B = 64
    states, ees = instances(cfg, config_b_instance, B)
    r = resync_protocol(cfg, states, ees, steps=12, step_rule=False, fused=True, min_alive=B - 2)
    c = r['counters']
    print('resync parity, reference criterion (0, 0) through the fused launch, 64 x 12: worst', r['worst'], c, 'device SolvedInacc at', r['inacc_where'],
          'duals on the row space in %d solves' % r['duals_compared_on_row_space'])
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL and r['worst']['z'] < REL_TOL and r['worst']['dual_obj'] <= 1e-6
    assert c['step_rule'] == 0 and c['low_tried'] == 0, c


def test_config_c_values_at_n20_entrywise():
    """BASELINE config 3 as written: a1_gait_opt_config.yaml values (mu 0.6, force bound 200, Q, swing 0.1, target x = y = 1) at
    N = 20, dt = 0.05 -- the RTI path of that configuration, 64 instances x 12 steps, entry-wise as above"""
    cfg = load_config('a1_gait_opt_config', num_nodes=20, integrator_dt=0.05)
    B = 64
    states, ees = instances(cfg, config_c_instance, B)
    r = resync_protocol(cfg, states, ees, steps=12, qp_every=2)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    print('resync parity, config C values 64 x 12: worst', r['worst'])


def test_config_d_n50_share_entrywise():
    """BASELINE config 4 (a1_config_distr_rejection.yaml: N = 50, dt = 0.02, pushes on the initial momentum): a 16-instance share of
    its 512 per GPU over 6 steps, entry-wise as above (the 3-rows-per-thread instance of the solve kernel)"""
    cfg = load_config('a1_config_distr_rejection')
    assert cfg['num_nodes'] == 50
    B = 16
    states, ees = instances(cfg, config_d_instance, B)
    r = resync_protocol(cfg, states, ees, steps=6, qp_every=2)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    print('resync parity, config D 16 x 6: alive', r['alive'], 'worst', r['worst'])


def test_trajectory_roundtrip_clone_and_evaluation():
    """GetTrajectory / SetWarmStartTrajectory / copy semantics / spline evaluation entries of the boundary"""
    cfg = load_config()
    B = 4
    states, ees = instances(cfg, config_b_instance, B)
    g, oracles = make_batch(cfg, states, ees)
    g.create_initial_run(states, ees)
    for b in range(B):
        oracles[b].initial_run(states[b], ees[b].reshape(4, 3))
    g.rti_advance(0, 3); g.synchronize()
    # value semantics: a clone continues exactly like the original, and is independent of it
    c = g.clone()
    g.rti_advance(3, 2); c.rti_advance(3, 2); g.synchronize(); c.synchronize()
    assert np.array_equal(g.qp_solution(), c.qp_solution()) and bytes(g.get_trajectory()) == bytes(c.get_trajectory())
    c.rti_advance(5, 1); c.synchronize()
    assert not np.array_equal(g.qp_solution(), c.qp_solution())
    # SetWarmStartTrajectory(GetTrajectory()) of another object: the next solve is bit-identical
    d = host.BatchMPC(cfg, B)
    d.set_solver_tolerances(*host.REFERENCE_SOLVER_SETTINGS)
    d.set_solver_step_rule(*g.solver_step_rule())       # (a new batch runs the reference's criterion; g was opted into the fast termination)
    d.set_warm_start_trajectory(g.get_trajectory())
    g.set_warm_start_trajectory(g.get_trajectory())     # (installing a trajectory also resets the solver's per-instance memory: the back-off of the
                                                        #  lower-start attempts -- g has five solves of history, d has none)
    tr = g.trajectory_states()
    t5 = 5 * cfg['integrator_dt']
    f, p, cont = g.eval_trajectory(t5)
    g.get_real_time_update(tr[:, 1], t5, p.reshape(B, 12))
    d.get_real_time_update(tr[:, 1], t5, p.reshape(B, 12))
    assert np.array_equal(g.qp_solution(), d.qp_solution())
    assert np.array_equal(g.sizes(), d.sizes())
    # device evaluation == host evaluation of the record == oracle spline on the oracle's own trajectory
    recs = g.get_trajectory()
    t = recs[0].init_time + 0.123
    f, p, cont = g.eval_trajectory(t)
    for b in range(B):
        for ee in range(4):
            # (same source on both sides; the device build contracts a*b + c into fused multiply-adds, x86-64 does not)
            assert np.allclose(recs[b].get_force(ee, t), f[b, ee], rtol=1e-12, atol=1e-12)
            assert np.allclose(recs[b].get_end_effector_location(ee, t), p[b, ee], rtol=1e-13, atol=1e-14)
            assert recs[b].get_contacts(t)[ee] == bool(cont[b, ee])
    o = oracles[0]
    rec_o = o.trajectory_record(host)
    for ee in range(4):
        for tt in (0.0, 0.07, 0.31, 0.77):
            assert np.allclose(rec_o.get_force(ee, tt), [o.ee_value(ee, 0, c_, tt) for c_ in range(3)], rtol=1e-12, atol=1e-12)
            assert np.allclose(rec_o.get_end_effector_location(ee, tt), [o.ee_value(ee, 1, c_, tt) for c_ in range(3)], rtol=1e-13, atol=1e-14)
    # a malformed record is refused
    bad = g.get_trajectory()
    bad[1].nk[2] = 1
    with pytest.raises(RuntimeError):
        g.set_warm_start_trajectory(bad)
    # GetEEBoxCenter = GetCOMToHip(ee).xy (SURVEY.md 8d constants), GetCost / GetAvgCost
    assert np.allclose(g.ee_box_center(), [[0.2055, 0.147], [0.2055, -0.147], [-0.1555, 0.147], [-0.1555, -0.147]], atol=1e-12)
    assert np.array_equal(g.cost(), g.stats()[:, 1])
    h = host.BatchMPC.cold_start(cfg, states[0], None, initial_run=False)
    costs = []
    for k in range(4):
        h.get_real_time_update(states[0], 0.0, ees[0])
        costs.append(h.cost()[0])
    assert abs(h.avg_cost()[0] - np.mean(costs)) <= 1e-12 * abs(np.mean(costs))


def test_sticky_error_accumulators_survive_multi_step_launches():
    """kernel 1 restarts err / status at every solve, so a K-step launch used to certify only its last step.
    The accumulators keep every bit and count the solves by outcome."""
    cfg = load_config()
    B = 8
    states, ees = instances(cfg, config_b_instance, B)
    g = host.BatchMPC.cold_start(cfg, states, ees)
    g.clear_status_accumulators()
    g.rti_advance(0, 6); g.synchronize()
    acc = g.status_accumulated()
    assert np.all(acc[:, 0] == 0) and np.all(acc[:, 1] == 6) and np.all(acc[:, 2] == 0)
    # an error raised BEFORE a solve (a lookup outside the knot range: the reference throws) is still visible after later solves
    f, p, c = g.eval_trajectory(np.full(B, -50.0))
    _, err = g.status()
    assert np.all(err & 1)                                   # SRBM_ERR_TIME_SMALL
    g.rti_advance(6, 2); g.synchronize()
    _, err = g.status()
    acc = g.status_accumulated()
    assert np.all(err == 0) and np.all(acc[:, 0] & 1) and np.all(acc[:, 1] == 8)
    g.clear_status_accumulators(); g.synchronize()
    assert np.all(g.status_accumulated() == 0)
    # a failed solve in the MIDDLE of a launch: an iteration limit of 3 makes every solve MaxIter; restore, run on
    g.set_solver_tolerances(1e-15, 1e-15, 1e-10, 3)
    g.rti_advance(8, 2); g.synchronize()
    g.set_solver_tolerances(*host.REFERENCE_SOLVER_SETTINGS)
    g.rti_advance(10, 3); g.synchronize()
    acc = g.status_accumulated()
    assert np.all(acc[:, 1] == 5) and np.all(acc[:, 2] >= 2) and np.all(acc[:, 3] >= 2)


def test_result_record_carries_primal_dual_and_contact_times():
    """SURVEY.md 8e record: {status, n, m, cost, alpha, err, iters, t, x[n], z[m], contact times} packed on the device"""
    cfg = load_config()
    B = 4
    states, ees = instances(cfg, config_b_instance, B)
    g = host.BatchMPC.cold_start(cfg, states, ees)
    g.rti_advance(0, 4); g.synchronize()
    LD = g.result_record_doubles()
    N = cfg['num_nodes']
    NX, NM = 12 * (N + 1) + 160, 12 * (N + 1) + 720 + 16 * (N - 3) + 16
    assert LD == 8 + NX + NM + 36
    r = g.pack_results()
    sz = g.sizes(); st, _ = g.status(); x = g.qp_solution(); z, _ = g.dual_solution(); stats = g.stats()
    trajs = g.get_trajectory()
    for b in range(B):
        n, m = int(sz[b, 0]), int(sz[b, 1])
        assert (r[b, 0], r[b, 1], r[b, 2]) == (st[b], n, m) and r[b, 3] == stats[b, 1] and r[b, 4] == stats[b, 0]
        assert np.array_equal(r[b, 8:8 + n], x[b, :n]) and np.all(r[b, 8 + n:8 + NX] == 0)
        assert np.array_equal(r[b, 8 + NX:8 + NX + m], z[b, :m]) and np.all(r[b, 8 + NX + m:8 + NX + NM] == 0)
        ct = trajs[b].get_contact_times()
        oc = 8 + NX + NM
        for ee in range(4):
            assert r[b, oc + ee] == len(ct[ee])
            assert np.array_equal(r[b, oc + 4 + 8 * ee: oc + 4 + 8 * ee + len(ct[ee])], ct[ee])
