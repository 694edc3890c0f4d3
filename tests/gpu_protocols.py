"""The two long drivers of the GPU tests, shared by several test modules (a plain module: nothing pytest collects).

    run_case                    a K-step launch against its one-step launches, bit for bit: test_gpu_launch_equivalence, test_gpu_dense_rows
    make_batch, resync_protocol the device re-synchronised to the oracle before every step, entry-wise parity: test_gpu_resync, test_gpu_dense_rows

Bodies and assertions are those the two modules held; the small helpers they use are in tests/gpu_kit.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from gpu_kit import REL_TOL, advance, assert_bitwise, relerr, snapshot
from gpu_kit import status_four_classes as cls
from cost_variants_kit import install
from oracle_py import OracleMPC
from srbm_loader import host
from srbm_loader.workloads import instances


def run_case(cfg, make_inst, B, steps, mode, splits, large=None, closed=False, prepare=None):
    """cold start, then the one-step chain and the split launches from clones of the same state; returns the chain's counter deltas.
    prepare(batch): called after the cold start (e.g. a contact schedule of its own)"""
    states, ees = instances(cfg, make_inst, B)
    base = host.BatchMPC.cold_start(cfg, states, ees, mode=mode, large=large)
    if prepare is not None:
        prepare(base)
    if closed:                                                     # the pushes of tests/test_gpu_queue.py
        base.plant_set_state(states)
        imp = np.zeros((B, 6)); imp[::7, 0] = 0.4; imp[::11, 1] = -0.3
        base.plant_set_push(time=np.full(B, 2.5 * cfg['integrator_dt']), impulse=imp)
    base.synchronize()
    c0 = base.solver_counters()
    chain = base.clone()
    ref = []
    for i in range(steps):
        advance(chain, closed, i, 1)
        chain.synchronize()
        info = chain.debug_launch_info()
        assert info['steps'] == 1 and not info['queued'], info
        ref.append(snapshot(chain, closed))
    n_cu = info['n_cu']
    c1 = chain.solver_counters()
    chain.close()
    assert all(sum(sp) == steps for sp in splits) and any(len(sp) == 1 for sp in splits)
    queued_launches = 0
    for sp in splits:
        c = base.clone()
        first = 0
        for k in sp:
            advance(c, closed, first, k)
            c.synchronize()
            info = c.debug_launch_info()
            assert info['steps'] == k and info['queued'] == (B > n_cu and k > 1), info
            queued_launches += info['queued']
            first += k
            assert_bitwise(snapshot(c, closed), ref[first - 1], 'split %s, after step %d' % (sp, first))
        c.close()
    base.close()
    d = {k: c1[k] - c0[k] for k in c0}
    if mode[1] > 0 and not closed:                                 # (no attempts at all otherwise)
        d['skipped_attempts'] = d['solves'] - d['low_tried']
    print('launch equivalence B=%d steps=%d mode=%s closed=%d: n_cu %d, multi-step launch kernel %s, queued launches %d, chain counters %s'
          % (B, steps, mode, closed, n_cu, info['kernel'], queued_launches, d))
    assert d['solves'] == B * steps
    return dict(counters=d, n_cu=n_cu, queued_launches=queued_launches, kernel=info['kernel'], sizes=[r['sizes'] for r in ref], err=[r['err'] for r in ref])


def make_batch(cfg, states, ees, step_rule=True, large=None, costs=None):
    """costs: one (des, Q, Phi, Phi_w) per instance (tests/cost_variants_kit.py), installed on the device through the three _each setters and on
    the oracles through set_costs; None: the costs of the constructors"""
    B = len(states)
    g = host.BatchMPC.cold_start(cfg, states, ees, large=large, initial_run=False)
    if costs is not None:
        assert len(costs) == B
        install(g, 0, costs)
    assert g.solver_step_rule() == (0.0, 0.0)   # a new batch: exactly the reference's criterion (gap 1e-15), include/srbm_rti.h
    if step_rule:
        g.enable_fast_termination()             # bench.py's step_rule_mode: tol_step 1e-5, start_mu 0.1 (the latter acts in srbm_rti_advance only)
    oracles = []
    for b in range(B):
        o = OracleMPC(cfg)
        if costs is not None:
            o.set_costs(*costs[b])
        o.set_warmstart(states[b])
        oracles.append(o)
    return g, oracles


def resync_protocol(cfg, states, ees, steps, qp_every=1, pool=None, step_rule=True, min_alive=None, fused=False, large=None, x_tol=REL_TOL, start_mu=None,
                    qp_extra=(), contact_phase=None, costs=None):
    """cold start on both sides, then `steps` open-loop RTI steps (test/gait_opt_playground.cpp:113-126) with the device
    re-synchronised to the oracle before every step; returns per-step statistics.  Asserts entry-wise parity.
    fused=False: the device steps through srbm_get_real_time_update (host-pointer entry, one launch per phase: the lower-start attempt is
    never made there).  fused=True: through srbm_rti_advance(i, 1) -- the device-resident launch bench.py times, which takes node 1 and the
    spline feet of the installed trajectory as its inputs and, with start_mu > 0, begins every solve with the lower-start ATTEMPT.
    The assembled QP and the duals are compared at the steps i % qp_every == 0 and at the steps in qp_extra; primal and states at every step.
    contact_phase: after the cold start the oracles' contact times are set that far apart (as many per foot as they have); the device takes the
    schedule over with the first installed trajectory.
    costs: per-instance cost sets (make_batch); the result then also tells the instances apart (x_compared_each, worst_each)."""
    B = len(states)
    N = cfg['num_nodes']
    dt = cfg['integrator_dt']
    g, oracles = make_batch(cfg, states, ees, step_rule, large, costs)
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
    xcmp_each = np.zeros(B, int)
    worst_each = [dict() for _ in range(B)]
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
        for b, r in enumerate(res):
            if r.get('dead'):
                n_gave_up += r.get('gave_up', 0); n_gave_up_cert += r.get('gave_up_cert', 0)
                worst['x_cert_gpu_where_oracle_gave_up'] = max(worst['x_cert_gpu_where_oracle_gave_up'], r.get('x_cert_gpu_where_oracle_gave_up', 0.0))
                continue
            total += 1
            exact_status += r['exact']
            seen_sizes.add(r['n']); seen_shapes.add((r['n'], r['nf'])); seen_td += r['ntd'] > 0
            n_xcmp += r.get('x_compared', 0)
            xcmp_each[b] += r.get('x_compared', 0)
            n_unique += r.get('z_unique', 0)
            n_cert += r.get('cert', 0)
            n_inacc += r.get('inacc', 0)
            n_atz += r.get('atz', 0)
            if 'inacc_where' in r:
                inacc_where.append(r['inacc_where'])
            for k in worst:
                if k in r:
                    worst[k] = max(worst[k], r[k])
                    worst_each[b][k] = max(worst_each[b].get(k, 0.0), r[k])
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
    return dict(inacc=n_inacc, inacc_where=inacc_where, duals_compared_on_row_space=n_atz, oracle_gave_up=n_gave_up, device_certified_where_oracle_gave_up=n_gave_up_cert, x_by_step=x_by_step, counters=ctr, alive=int(alive.sum()), sizes=seen_sizes, shapes=seen_shapes, x_compared=n_xcmp, x_compared_each=xcmp_each, worst_each=worst_each, td_steps=seen_td, worst=worst, exact_status=exact_status, total=total, z_unique=n_unique, certified=n_cert)
