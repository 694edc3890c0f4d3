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
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle_py import OracleMPC, load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, config_c_instance, config_d_instance

pytestmark = pytest.mark.gpu
REL_TOL = 1e-4
EE0 = np.array([[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]], float)


def relerr(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def cls(v):
    v = int(v)
    return 'solved' if v <= 1 else ('maxiter' if v == 2 else ('infeasible' if v in (3, 5) else 'other'))


def make_batch(cfg, states, ees, step_rule=True, large=None):
    B = len(states)
    g = host.BatchMPC(cfg, B, large=large)
    g.set_state_trajectory_warm_start(states)
    g.set_solver_tolerances(1e-15, 1e-15, 1e-10, 200)
    assert g.solver_step_rule() == (0.0, 0.0)   # a new batch: exactly the reference's criterion (gap 1e-15), include/srbm_rti.h
    if step_rule:
        g.enable_fast_termination()             # bench.py's step_rule_mode: tol_step 1e-5, start_mu 0.1 (the latter acts in srbm_rti_advance only)
    oracles = []
    for b in range(B):
        o = OracleMPC(cfg)
        o.set_warmstart(states[b])
        oracles.append(o)
    return g, oracles


def resync_protocol(cfg, states, ees, steps, qp_every=1, pool=None, step_rule=True, min_alive=None, fused=False, large=None, x_tol=REL_TOL, start_mu=None,
                    qp_extra=(), contact_phase=None):
    """cold start on both sides, then `steps` open-loop RTI steps (test/gait_opt_playground.cpp:113-126) with the device
    re-synchronised to the oracle before every step; returns per-step statistics.  Asserts entry-wise parity.
    fused=False: the device steps through srbm_get_real_time_update (host-pointer entry, one launch per phase: the lower-start attempt is
    never made there).  fused=True: through srbm_rti_advance(i, 1) -- the device-resident launch bench.py times, which takes node 1 and the
    spline feet of the installed trajectory as its inputs and, with start_mu > 0, begins every solve with the lower-start ATTEMPT.
    The assembled QP and the duals are compared at the steps i % qp_every == 0 and at the steps in qp_extra; primal and states at every step.
    contact_phase: after the cold start the oracles' contact times are set that far apart (as many per foot as they have); the device takes the
    schedule over with the first installed trajectory."""
    B = len(states)
    N = cfg['num_nodes']
    dt = cfg['integrator_dt']
    g, oracles = make_batch(cfg, states, ees, step_rule, large)
    if start_mu is not None:
        g.set_solver_step_rule(g.solver_step_rule()[0], start_mu)
    x_by_step = []
    pool = pool or ThreadPoolExecutor(16)
    list(pool.map(lambda b: oracles[b].initial_run(states[b], ees[b].reshape(4, 3)), range(B)))
    g.create_initial_run(states, ees.reshape(B, 12))
    g.clear_status_accumulators()              # (the counters below describe the re-synchronised steps only)
    # after the cold start (10 solves, each side on its own path) the two sides agree to the tolerance ...
    xs = g.qp_solution()
    st0, _ = g.status()
    for b in range(B):
        so = oracles[b].stats()['status']
        assert cls(st0[b]) == cls(so) or {cls(st0[b]), cls(so)} <= {'solved', 'maxiter'}, (b, st0[b], so)
    if contact_phase is not None:
        for o in oracles:
            o.set_contact_times([contact_phase * np.arange(len(o.contact_times(e)[0])) for e in range(4)])
    seen_sizes, seen_td, worst = set(), 0, dict(A=0.0, x=0.0, x_inacc=0.0, z=0.0, z_all=0.0, Atz=0.0, states=0.0, x_cert_oracle=0.0, x_cert_gpu=0.0, x_cert_gpu_where_oracle_gave_up=0.0,
                                               dual_obj=0.0, kkt=0.0)
    n_cert = 0
    n_xcmp = 0
    seen_shapes = set()          # (n, n_force) of the compared solves
    n_inacc = 0
    n_atz = 0
    n_gave_up = n_gave_up_cert = 0
    inacc_where = []
    n_unique = 0
    exact_status = 0
    total = 0
    nx = (N + 1) * 12
    # An instance leaves the comparison when the ORACLE's solver gives up on it (MaxIterations / numerical error: its iterate is
    # then not a minimiser and the trajectory it continues from is solver-specific, cf. tests/test_gpu_parity.py); the device
    # keeps running that instance on its own trajectory.
    alive = np.ones(B, bool)
    for i in range(steps):
        t = i * dt
        # ... and from here on the device starts every step from the ORACLE's trajectory
        own = g.get_trajectory()
        recs = (host.Trajectory * B)(*[oracles[b].trajectory_record(host) if alive[b] else own[b] for b in range(B)])
        g.set_warm_start_trajectory(recs)
        back = g.get_trajectory()
        assert bytes(back) == bytes(recs)                      # the record round-trips bit for bit
        own_states = g.trajectory_states()
        _, own_ee, _ = g.eval_trajectory(t)
        # (fused: the launch reads node 1 of the installed trajectory at every step, the first included -- the oracle is given the same)
        st_in = np.array([(o.states()[1] if (i > 0 or fused) else states[b]) if alive[b] else own_states[b, 1] for b, o in enumerate(oracles)])
        ee_in = np.array([[[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)] if alive[b] else own_ee[b]
                          for b, o in enumerate(oracles)]).reshape(B, 12)
        if fused:
            g.rti_advance(i, 1); g.synchronize()
            if g.solver_step_rule()[1] > 0:       # every solve of this launch began with an attempt (installing a trajectory resets the back-off)
                fl = g.solve_flags()
                assert np.all(fl & 2), (i, np.nonzero((fl & 2) == 0)[0][:8])
        else:
            g.get_real_time_update(st_in, t, ee_in)
        sos = list(pool.map(lambda b: oracles[b].rti(st_in[b], t, ee_in[b].reshape(4, 3)) if alive[b] else 8, range(B)))
        sz = g.sizes(); st, err = g.status(); stats = g.stats()
        x = g.qp_solution(); xr = g.raw_qp_minimiser(); z, s = g.dual_solution(); tr = g.trajectory_states()
        assert np.all(err[alive] == 0), (i, np.nonzero(err)[0][:8], err[err != 0][:8])
        traj_after = g.get_trajectory()
        qp_step = i % qp_every == 0 or i in qp_extra

        def check(b):
            o = oracles[b]
            if not alive[b]:
                return dict(exact=0, n=0, ntd=0, dead=1)
            if cls(sos[b]) in ('maxiter', 'other'):
                # The ORACLE's solver gives up on this QP (its iterate is not a minimiser, the instance leaves the comparison from here on) -- but the
                # DEVICE's answer to it is still checked: where the device reports Solved, its minimiser is certified independently of both
                # interior-point codes (tests/qp_polish.py: active-set polish of the device's own point on the device's exported QP + KKT certificate)
                alive[b] = False
                gave = dict(exact=0, n=0, ntd=0, dead=1, gave_up=1)
                if int(st[b]) == 0:
                    from qp_polish import polish
                    A, bv, P, q = g.export_qp(b)
                    n_, m_ = int(sz[b, 0]), int(sz[b, 1])
                    is_eq = np.ones(m_, bool)
                    is_eq[nx:nx + int(sz[b, 3])] = False
                    xc, info = polish(P, q, A, bv, is_eq, xr[b, :n_], z[b, :m_], s[b, :m_])
                    if xc is not None:
                        gave['gave_up_cert'] = 1
                        gave['x_cert_gpu_where_oracle_gave_up'] = relerr(xr[b, :n_], xc)
                        assert gave['x_cert_gpu_where_oracle_gave_up'] < REL_TOL, (i, b, gave['x_cert_gpu_where_oracle_gave_up'])
                return gave
            osz = o.sizes()
            n, m = osz['n'], osz['m']
            assert (sz[b, 0], sz[b, 1], sz[b, 2], sz[b, 3], sz[b, 4], sz[b, 5], sz[b, 6]) == \
                   (n, m, osz['n_eq'], osz['n_ineq'], osz['n_force'], osz['n_pos'], osz['n_td']), (i, b)
            co, cg = cls(sos[b]), cls(st[b])
            # Solved / SolvedInacc / MaxIter steer the RTI step identically (msrb.cpp:136-144); which of them an IPM reports at a
            # 1e-15 gap tolerance is solver-internal (Clarabel is unpinned).  Infeasible must match exactly.
            assert co == cg or {co, cg} <= {'solved', 'maxiter'}, (i, b, sos[b], st[b])
            out = dict(exact=int(int(sos[b]) == int(st[b])), n=n, nf=osz['n_force'], ntd=osz['n_td'])
            # knot tables after the step (horizon shift of this step included): bit-exact
            ta = traj_after[b]
            for ee in range(4):
                ko = o.knots(ee)
                K = ko['K']
                assert ta.nk[ee] == K, (i, b, ee)
                assert np.array_equal(np.array(ta.knot_time[ee][:K]), ko['times']), (i, b, ee)
            if qp_step:
                A, bv, P, q = g.export_qp(b)
                Ao, bo, Po, qo = o.qp_dense()
                # sparsity pattern: identical above rounding noise.  (The reference's SetMatrix drops EXACT zeros,
                # sparse_matrix_builder.cpp:22-30; a spline value that is 0.0 on one side and 1e-16 on the other -- a force at
                # a lift-off knot, evaluated with and without fused multiply-adds -- moves an entry in or out of the pattern
                # without changing the QP; the t = 0 test of tests/test_gpu_parity.py keeps the exact-pattern check.)
                # (with a band around the threshold: an entry of 1.1e-13 on one side and 0.9e-13 on the other is the same entry)
                assert not np.any((np.abs(A) > 1e-12) & (np.abs(Ao) <= 1e-14)) and not np.any((np.abs(Ao) > 1e-12) & (np.abs(A) <= 1e-14)), (i, b)
                out['A'] = max(np.abs(A - Ao).max(), np.abs(bv - bo).max(), np.abs(P - Po).max(), np.abs(q - qo).max())
                assert out['A'] <= 1e-12, (i, b, out['A'])
            if co == 'infeasible':      # sol := prev_qp_sol (msrb.cpp:115-120): the step is zero on both sides
                assert stats[b, 0] * stats[b, 3] == 0.0 or stats[b, 3] < 1e-12, (i, b)
                return out
            if co != 'solved' or cg != 'solved':
                return out              # an unconverged QP: the iterate it stopped at is solver-specific
            xo = o.x()
            out['x'] = max(relerr(xr[b, :n], o.qp_x()), relerr(x[b, :n], xo))
            out['x_compared'] = 1
            if int(st[b]) == 1:
                # the DEVICE itself reports SolvedInacc where the oracle reports Solved: counted, located, and held to the SAME bound as every other
                # pair (round 4 allowed 10 x here)
                out['inacc'] = 1
                out['x_inacc'] = out['x']
                out['inacc_where'] = (i, b, int(stats[b, 4]), float(out['x']))
            assert out['x'] < x_tol, (i, b, out['x'], int(st[b]), int(sos[b]))
            out['states'] = relerr(tr[b], o.states())
            assert out['states'] < x_tol, (i, b)
            # a sample is checked against the CERTIFIED minimiser of the QP (tests/qp_polish.py: active-set polish + KKT
            # certificate, independent of both interior-point codes): the oracle's minimiser is pinned by it, the device's too
            if qp_step and (b + 5 * i) % 64 == 0:
                from qp_polish import polish
                is_eq = np.ones(m, bool)
                is_eq[nx:nx + osz['n_ineq']] = False
                xc, info = polish(Po, qo, Ao, bo, is_eq, o.qp_x(), o.z(), o.s())
                if xc is not None:
                    out['cert'] = 1
                    out['x_cert_oracle'] = relerr(o.qp_x(), xc)
                    out['x_cert_gpu'] = relerr(xr[b, :n], xc)
                    assert out['x_cert_oracle'] < REL_TOL and out['x_cert_gpu'] < REL_TOL, (i, b, out['x_cert_oracle'], out['x_cert_gpu'])
            # duals.  Always: the device's (x, z) is a KKT point of the ORACLE's QP (stationarity, sign, complementarity) and the
            # dual objectives agree.  Entry-wise z == z_oracle only where the multipliers are unique, i.e. where the gradients
            # of the active rows are linearly independent (a foot with zero force has its lower force-box row and its four
            # pyramid rows active together: five dependent rows, any split of the multiplier is optimal).
            if qp_step:
                zo, so_ = o.z(), o.s()
                zg, sg = z[b, :m], s[b, :m]
                xg = xr[b, :n]
                zs = max(1.0, np.abs(zo).max())
                # stationarity of the device's (x, z) on the oracle's QP.  At the gap criterion 1e-7 of |q|; a solve that ends through the step rule
                # takes its last (affine) step without a corrector, which leaves the multipliers accurate to the order of the primal bound
                # (DESIGN.md section 3), i.e. to the north-star tolerance: 1e-4 there (observed worst 1.2e-6 at N = 20; at N = 40 on the LARGE build one solve sits
                # at 1e-5 ... 2.4e-5 and moves inside that band with rounding-level changes of the assembly -- round 4 asserted 1e-5 on an observed 9.8e-6)
                out['kkt'] = np.abs(Po @ xg + qo + Ao.T @ zg).max() / max(1.0, np.abs(qo).max())
                assert out['kkt'] < (REL_TOL if step_rule else 1e-7), (i, b, out['kkt'])
                n_eq0 = nx                               # dynamics rows first, then the inequality blocks, then TD / start rows
                ineq = slice(nx, nx + osz['n_ineq'])
                assert zg[ineq].min() > -1e-7 * zs and sg[ineq].min() > -1e-9, (i, b)
                assert np.abs(zg[ineq] * sg[ineq]).max() < 1e-6 * zs, (i, b)
                # dual objective b'z: a sum of terms of both signs (|b'z| ~ 1e2 out of terms b_i z_i of 1e4 and more).  At the reference's gap
                # criterion (step_rule=False) both sides agree to 1e-6 OF THE SUM, which is a 1e-8 statement on the multipliers.  The step rule
                # (the default of the library) bounds the primal distance to the minimiser (5e-6 relative) and leaves the
                # multipliers accurate to that order: the sum then agrees to 1e-6 of the magnitude of its TERMS -- asserted as such
                dscale = abs(bo @ zo) if not step_rule else np.abs(bo * zo).sum()
                out['dual_obj'] = abs(bo @ zg - bo @ zo) / max(1.0, abs(bo @ zo))
                assert abs(bo @ zg - bo @ zo) <= 1e-6 * max(1.0, dscale), (i, b, bo @ zg, bo @ zo, dscale)
                # the IDENTIFIABLE part of the multipliers, for EVERY solve: A'z is determined by stationarity (A'z = -(P x + q)) whatever split of
                # dependent active rows a solver picked -- the projection of z_gpu - z_oracle onto the row space of the constraint matrix
                out['Atz'] = np.abs(Ao.T @ (zg - zo)).max() / max(1.0, np.abs(Ao.T @ zo).max())
                out['atz'] = 1
                assert out['Atz'] < REL_TOL, (i, b, out['Atz'])
                active = np.ones(m, bool)
                active[ineq] = so_[ineq] < 1e-7
                active &= np.abs(Ao).sum(axis=1) > 0      # rows without coefficients constrain nothing
                Aact = Ao[active]
                out['z_all'] = np.abs(zg[active] - zo[active]).max() / zs
                # (the rank test is the expensive part: a sample of the solves)
                if (b + i) % 4 == 0 and np.linalg.matrix_rank(Aact, tol=1e-9) == Aact.shape[0]:
                    out['z'] = out['z_all']
                    out['z_unique'] = 1
                    assert out['z'] < REL_TOL, (i, b, out['z'])
            os_ = o.stats()
            if os_['step_norm'] > 1e-3:           # the Armijo test is noise below that (merit differences ~1e-12)
                assert stats[b, 0] == os_['alpha'], (i, b, stats[b, 0], os_['alpha'])
            assert abs(stats[b, 1] - os_['cost']) <= 1e-6 * max(1.0, abs(os_['cost'])), (i, b)
            return out

        res = list(pool.map(check, range(B)))
        xs_ = np.array([r.get('x', 0.0) for r in res])
        x_by_step.append((float(xs_.max()), int(xs_.argmax()), int((xs_ > REL_TOL).sum())))
        for r in res:
            if r.get('dead'):
                n_gave_up += r.get('gave_up', 0); n_gave_up_cert += r.get('gave_up_cert', 0)
                worst['x_cert_gpu_where_oracle_gave_up'] = max(worst['x_cert_gpu_where_oracle_gave_up'], r.get('x_cert_gpu_where_oracle_gave_up', 0.0))
                continue
            total += 1
            exact_status += r['exact']
            seen_sizes.add(r['n']); seen_shapes.add((r['n'], r['nf'])); seen_td += r['ntd'] > 0
            n_xcmp += r.get('x_compared', 0)
            n_unique += r.get('z_unique', 0)
            n_cert += r.get('cert', 0)
            n_inacc += r.get('inacc', 0)
            n_atz += r.get('atz', 0)
            if 'inacc_where' in r:
                inacc_where.append(r['inacc_where'])
            for k in worst:
                if k in r:
                    worst[k] = max(worst[k], r[k])
        # foot-box size (info_.ee_box_size, grown / shrunk by the status of each solve): same on both sides
        for b in (0, B // 2, B - 1):
            if alive[b]:
                assert np.array_equal(g.knots(b)['box'], np.array(oracles[b].stats()['box'])), (i, b)
    assert alive.sum() >= (0.97 * B if min_alive is None else min_alive), alive.sum()
    ctr = g.solver_counters()
    assert ctr['solves'] == B * steps
    if fused and g.solver_step_rule()[1] > 0:  # the test cannot silently run without attempts
        assert ctr['low_tried'] >= 0.8 * ctr['solves'], ctr
    # (a device SolvedInacc where the oracle says Solved is a CLASSIFICATION difference of two interior-point codes at the fp64 floor -- observed on 13 of
    #  5 102 host-driven solves, all within 6e-11 of the oracle's minimiser; every such pair is held to the full bound above and listed in the result)
    return dict(inacc=n_inacc, inacc_where=inacc_where, duals_compared_on_row_space=n_atz, oracle_gave_up=n_gave_up, device_certified_where_oracle_gave_up=n_gave_up_cert, x_by_step=x_by_step, counters=ctr, alive=int(alive.sum()), sizes=seen_sizes, shapes=seen_shapes, x_compared=n_xcmp, td_steps=seen_td, worst=worst, exact_status=exact_status, total=total, z_unique=n_unique, certified=n_cert)


def test_config_b_all_256_instances_entrywise_over_20_steps():
    """the full protocol at the REFERENCE'S criterion (a new batch: srbm_set_solver_step_rule(0, 0)), host-driven (srbm_get_real_time_update): all 256
    instances x 20 steps with the strict dual bounds -- dual objective to 1e-6 of its value, stationarity 1e-7.  The bench mode has the same
    protocol through the fused launch below; the step rule on the host-driven path is covered by the Config-C / Config-D runs"""
    cfg = load_config()
    B = 256
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_d_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
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
    states, ees = zip(*[config_c_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
    r = resync_protocol(cfg, states, ees, steps=12, qp_every=2)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    print('resync parity, config C values 64 x 12: worst', r['worst'])


def test_config_d_n50_share_entrywise():
    """BASELINE config 4 (a1_config_distr_rejection.yaml: N = 50, dt = 0.02, pushes on the initial momentum): a 16-instance share of
    its 512 per GPU over 6 steps, entry-wise as above (the 3-rows-per-thread instance of the solve kernel)"""
    cfg = load_config('a1_config_distr_rejection')
    assert cfg['num_nodes'] == 50
    B = 16
    states, ees = zip(*[config_d_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees)
    r = resync_protocol(cfg, states, ees, steps=6, qp_every=2)
    assert r['worst']['A'] <= 1e-12 and r['worst']['x'] < REL_TOL
    print('resync parity, config D 16 x 6: alive', r['alive'], 'worst', r['worst'])


def test_trajectory_roundtrip_clone_and_evaluation():
    """GetTrajectory / SetWarmStartTrajectory / copy semantics / spline evaluation entries of the boundary"""
    cfg = load_config()
    B = 4
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees).reshape(B, 12)
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
    d.set_solver_tolerances(1e-15, 1e-15, 1e-10, 200)
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
    h = host.BatchMPC(cfg, 1)
    h.set_state_trajectory_warm_start(states[0]); h.set_solver_tolerances(1e-15, 1e-15, 1e-10, 200)
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
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees).reshape(B, 12)
    g = host.BatchMPC(cfg, B)
    g.set_state_trajectory_warm_start(states)
    g.create_initial_run(states, ees)
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
    g.set_solver_tolerances(1e-15, 1e-15, 1e-10, 200)
    g.rti_advance(10, 3); g.synchronize()
    acc = g.status_accumulated()
    assert np.all(acc[:, 1] == 5) and np.all(acc[:, 2] >= 2) and np.all(acc[:, 3] >= 2)


def test_result_record_carries_primal_dual_and_contact_times():
    """SURVEY.md 8e record: {status, n, m, cost, alpha, err, iters, t, x[n], z[m], contact times} packed on the device"""
    cfg = load_config()
    B = 4
    states, ees = zip(*[config_b_instance(cfg, b) for b in range(B)])
    states, ees = np.array(states), np.array(ees).reshape(B, 12)
    g = host.BatchMPC(cfg, B)
    g.set_state_trajectory_warm_start(states)
    g.create_initial_run(states, ees)
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
