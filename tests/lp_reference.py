"""The contact-time LP of the gait step stated plainly and solved exactly: the reference of tests/test_gpu_gait_lp.py.

    build_lp        the rows of GaitOptimizer::CreatePolytopeConstraint, CreateStartConstraint, CreateTrustRegionConstraint (Delta = 1) and
                    CreateNextNodeConstraints (gait_optimizer.cpp:410-534) as dense matrices, written from that text
    solve_lp        scipy's dual simplex on them, with a certificate of its answer computed here in numpy
    value_bound     what the device's documented stop test allows between its value and the exact one (derivation there)
    vertex_rows     the rows that pin the minimiser down, and whether they pin all of it
    draw_case, draw_cases     the seeded schedules, times and gradients the GPU test runs (generated on the host, no device involved)

A plain module: no kernel code, no oracle code, nothing pytest collects."""
import numpy as np
from scipy.optimize import linprog

LO, TD, F, MID = 0, 1, 2, 3          # knot kinds of a trajectory record (include/srbm_rti.h); LiftOff / TouchDown of the reference's TimeType
MIN_TIME = 0.2                       # gait_optimizer.cpp:412
DELTA = 1.0                          # the trust region the reference is left with (its updates are commented out, gait_optimizer.cpp:199-211)
CERT_TOL = 1e-12                     # a reference is certified to this fraction of max(1, |c|_inf)


def next_node(ct, tnow):
    """first index >= 1 whose contact time is >= tnow (gait_optimizer.cpp:419-425, 515-521); None where there is none -- the reference then
    evaluates contact_times_.at(ee).at(-1) and throws"""
    for j in range(1, len(ct)):
        if ct[j] >= tnow:
            return j
    return None


def build_lp(cts, kinds, tnow):
    """(A_ub, b_ub, A_eq, b_eq) over the step s of all contact times, foot after foot (GetNumTimeNodes(ee) is the offset of foot ee).
    cts[ee]: contact times of foot ee, kinds[ee]: LO / TD of each.  Every two-sided row lb <= a's <= ub of the reference becomes a's <= ub
    and -a's <= -lb; its equalities (lb == ub == 0) stay equalities.
    A foot whose contact times all lie before tnow has no next node: the reference throws there (see next_node); the rows stated here are then
    those that do not depend on the next node, i.e. no next-node rows for that foot and the plain polytope row between all its neighbours."""
    counts = [len(c) for c in cts]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    nv = int(offs[-1])
    ub_rows, ub_rhs, eq_rows = [], [], []

    def two_sided(a, lb, ub):
        ub_rows.append(a); ub_rhs.append(ub)
        ub_rows.append(-a); ub_rhs.append(-lb)

    def unit(j, v=1.0):
        a = np.zeros(nv); a[j] = v
        return a

    # CreatePolytopeConstraint: s_{i-1} - s_i in [lb, ub] between neighbours, the last node's step in [0, 1]
    for ee in range(len(cts)):
        ct, o, n = np.asarray(cts[ee], float), offs[ee], counts[ee]
        nn = next_node(ct, tnow)
        nn_td = nn is not None and kinds[ee][nn] == TD
        for i in range(1, n):
            a = unit(o + i - 1) - unit(o + i)
            if i == nn and nn_td:
                two_sided(a, -3.0, ct[nn] - ct[nn - 1])               # "Constrained - no min time requirement"
            else:
                two_sided(a, -2.0, ct[i] - ct[i - 1] - MIN_TIME)
        two_sided(unit(o + n - 1), 0.0, 1.0)
    # CreateStartConstraint: the first contact time of a foot never moves
    for ee in range(len(cts)):
        eq_rows.append(unit(offs[ee]))
    # CreateTrustRegionConstraint, infinity norm
    for j in range(nv):
        two_sided(unit(j), -DELTA, DELTA)
    # CreateNextNodeConstraints: the two contact times around the next touch-down are frozen
    for ee in range(len(cts)):
        nn = next_node(np.asarray(cts[ee], float), tnow)
        if nn is not None and kinds[ee][nn] == TD:
            eq_rows.append(unit(offs[ee] + nn - 1))
            eq_rows.append(unit(offs[ee] + nn))
    A_ub, b_ub = np.array(ub_rows), np.array(ub_rhs, float)
    A_eq = np.array(eq_rows)
    return A_ub, b_ub, A_eq, np.zeros(len(eq_rows))


def solve_lp(c, A_ub, b_ub, A_eq, b_eq):
    """min c's over the rows of build_lp with scipy.optimize.linprog(method='highs-ds'), both feasibility tolerances at 1e-10.
    -> dict(feasible, x, f, y (marginals of the inequality rows, >= 0), z (of the equality rows), primal, dual, sign, gap, certified):
    the stationarity the marginals satisfy is c + A_ub' y + A_eq' z = 0, and the certificate -- all in numpy, independent of the solver's
    own report -- is  primal = worst row violation,  dual = |c + A_ub' y + A_eq' z|_inf,  sign = -min(y, 0),  gap = |c's - (-b_ub' y - b_eq' z)|.
    certified: every one of them <= CERT_TOL max(1, |c|_inf).  An LP the solver calls infeasible returns feasible = False and nothing else;
    any other outcome than optimal / infeasible raises (a reference that cannot be had is an error of the test)."""
    c = np.asarray(c, float)
    res = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=(None, None), method='highs-ds',
                  options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10))
    if res.status == 2:
        return dict(feasible=False)
    if res.status != 0:
        raise RuntimeError('linprog: ' + res.message)
    x = res.x
    y, z = -res.ineqlin.marginals, -res.eqlin.marginals
    C = max(1.0, np.abs(c).max())
    out = dict(feasible=True, x=x, f=float(c @ x), y=y, z=z,
               primal=max(0.0, (A_ub @ x - b_ub).max(), np.abs(A_eq @ x - b_eq).max()),
               dual=np.abs(c + A_ub.T @ y + A_eq.T @ z).max(), sign=max(0.0, -y.min()),
               gap=abs(c @ x + b_ub @ y + b_eq @ z))
    out['certified'] = max(out['primal'], out['dual'], out['sign'], out['gap']) <= CERT_TOL * C
    return out


def value_bound(c, marginals, nv, m):
    """E with |c's_dev - f*| <= E for every s_dev the device may stop at.

    The kernel stops at an iterate (s, t, l) -- step, slacks t > 0, multipliers l > 0 over its m rows A s <= b -- with
        mu = t'l / m < 1e-11 C,     |A s + t - b|_inf < 1e-10,     |c + A'l|_inf < 1e-10 C  on the variables that move,     C = max(1, |c|_inf),
    pinned variables held at exactly 0 (csrc/srbm_gait_lp.hiph).  Let s* be a minimiser, f* = c's*, and (y, z) the reference's marginals:
    c + A'y + A_eq'z = 0, y >= 0, y'(b - A s*) = 0.  Every step has |s_i| <= 1 (trust region), so |s|_1 <= nv.
      below:  c's_dev = -y'A s_dev - z'A_eq s_dev = -y'b + y'(b - A s_dev) = f* + y'(t - r) with |r|_inf < 1e-10 (the pinned entries are exact
              zeros, so the equality term vanishes), hence   c's_dev - f* >= -1e-10 |y|_1.
      above:  c's_dev = (c + A'l)'s_dev - l'(b - t + r)  and  c's* = (c + A'l)'s* - l'A s* >= (c + A'l)'s* - l'b  (weak duality: A s* <= b, l >= 0), so
              c's_dev - f* <= 1e-10 C (|s_dev|_1 + |s*|_1) + t'l + 1e-10 |l|_1 <= 2 nv 1e-10 C + m 1e-11 C + 1e-10 |l|_1.
    The device's multipliers are not exported; at the solution they are the marginals of the same LP, whose size |y|_1 + |z|_1 stands in for
    |l|_1 (the device has no equality rows: what z carries in the reference sits on the rows next to a pinned variable there) -- with the
    factor 2 on that term covering both sides and the stand-in:
        E = m 1e-11 C + 2 1e-10 (|y|_1 + |z|_1) + 2 nv 1e-10 C."""
    C = max(1.0, np.abs(np.asarray(c, float)).max()) if len(c) else 1.0
    return m * 1e-11 * C + 2 * 1e-10 * np.abs(marginals).sum() + 2 * nv * 1e-10 * C


def lane_rows(counts):
    """rows the kernel's lane layout carries: per contact time its two trust-region rows, per neighbour pair two polytope rows, per foot the two
    rows of the final-node box = 4 per contact time"""
    return 4 * int(np.sum(counts))


def pinned_columns(A_eq):
    return np.abs(A_eq).sum(axis=0) > 0


def vertex_rows(ref, A_ub, A_eq, tau):
    """(rows, nondegenerate): the inequality rows whose marginal is >= tau, and whether they determine every variable that moves -- their
    restriction to the unpinned columns has full column rank, which is the case the count "rows >= free variables" stands for at a vertex
    (rank instead of the count, so that the two identical rows s_last <= 1 of the trust region and of the final-node box, or a row between two
    pinned variables, cannot make up the number)"""
    rows = np.nonzero(ref['y'] >= tau)[0]
    free = ~pinned_columns(A_eq)
    if free.sum() == 0:
        return rows, True
    if len(rows) < free.sum():
        return rows, False
    return rows, np.linalg.matrix_rank(A_ub[np.ix_(rows, free)]) == free.sum()


# ---- the seeded cases of tests/test_gpu_gait_lp.py ----
COUNTS = [(2, 2, 2, 2), (4, 4, 4, 4), (3, 5, 2, 7), (16, 2, 2, 2), (2, 2, 2, 16), (2, 16, 2, 12), (8, 8, 8, 8), (16, 8, 4, 4)]
TIMES = ['inside', 'before', 'equal', 'td_first', 'td_last', 'lift_off', 'after']
GRADS = ['generic', 'spread', 'zeros']
KMAX = 32                            # knots a record holds per foot


def draw_schedule(rng, counts):
    """per foot: first contact time in [-0.3, 0], gaps uniform in [0.12, 0.6] (about one in six below the 0.2 s minimum phase), kinds
    alternating from a random start"""
    cts, kinds = [], []
    for k in counts:
        t = rng.uniform(-0.3, 0.0) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.12, 0.6, k - 1))])
        cts.append(t)
        kinds.append((np.arange(k) + rng.integers(2)) % 2)
    return cts, kinds


def draw_time(rng, cts, kinds, how):
    """the time of the LP; the targeted cases pick a foot, and flip its kinds where the case needs a touch-down / lift-off at a given index"""
    first, last = min(c[0] for c in cts), max(c[-1] for c in cts)
    ee = int(rng.integers(len(cts)))
    ct, k = cts[ee], len(cts[ee])
    if how == 'inside':
        return rng.uniform(first, last)
    if how == 'before':
        return first - 0.1
    if how == 'after':
        return last + 0.1
    if how == 'equal':
        return float(ct[rng.integers(1, k)])                     # bit-equal to a contact time: ct >= tnow holds with equality
    if how == 'td_first':
        j = 1
    elif how == 'td_last':
        j = k - 1
    else:
        j = int(rng.integers(1, k))
    want = LO if how == 'lift_off' else TD
    if kinds[ee][j] != want:
        kinds[ee] = 1 - kinds[ee]
    return rng.uniform(ct[j - 1], ct[j]) if ct[j - 1] < ct[j] else float(ct[j])


def draw_gradient(rng, nv, how):
    """generic: normal * 10**U(-2, 5); spread: the same with per-entry factors 10**U(-3, 3); zeros: generic with about a quarter of the entries 0.0"""
    c = rng.normal(size=nv) * 10 ** rng.uniform(-2, 5)
    if how == 'spread':
        c = c * 10 ** rng.uniform(-3, 3, nv)
    elif how == 'zeros':
        c[rng.random(nv) < 0.25] = 0.0
    elif how == 'all_zero':
        c[:] = 0.0
    return c


def knot_table(rng, ct, kinds, interleave):
    """(kinds, times) of a foot's knot table holding these contact knots; interleave: with the stance-interior knots F, F between a touch-down
    and the lift-off after it and the mid-swing knot MID between a lift-off and the next touch-down (knot times non-decreasing), so that a scan
    for contact knots has knots to skip.  Contact knots only where the table would not fit KMAX."""
    k = len(ct)
    if not interleave or 3 * k - 2 > KMAX:
        return np.asarray(kinds, int), np.asarray(ct, float)
    kk, tt = [], []
    for i in range(k):
        kk.append(int(kinds[i])); tt.append(float(ct[i]))
        if i + 1 < k:
            if kinds[i] == TD:
                kk += [F, F]; tt += [ct[i] + (ct[i + 1] - ct[i]) / 3, ct[i] + 2 * (ct[i + 1] - ct[i]) / 3]
            else:
                kk += [MID]; tt += [ct[i] + (ct[i + 1] - ct[i]) / 2]
    return np.array(kk, int), np.array(tt, float)


def draw_case(rng, counts, time_how, grad_how, interleave):
    """one LP with its reference: dict(counts, cts, kinds, tnow, c, table (per foot (kinds, times)), lp, ref, nv, m, and for a feasible one
    E, tau, rows, nondegenerate)"""
    cts, kinds = draw_schedule(rng, counts)
    tnow = draw_time(rng, cts, kinds, time_how)
    nv = int(np.sum(counts))
    c = draw_gradient(rng, nv, grad_how)
    table = [knot_table(rng, cts[e], kinds[e], interleave) for e in range(len(counts))]
    return make_case(counts, cts, kinds, tnow, c, table, time_how, grad_how)


def make_case(counts, cts, kinds, tnow, c, table, time_how='', grad_how=''):
    nv = int(np.sum(counts))
    lp = build_lp(cts, kinds, tnow)
    ref = solve_lp(c, *lp)
    case = dict(counts=tuple(counts), cts=cts, kinds=kinds, tnow=float(tnow), c=np.asarray(c, float), table=table, lp=lp, ref=ref, nv=nv,
                m=lane_rows(counts), time_how=time_how, grad_how=grad_how)
    if ref['feasible']:
        assert ref['certified'], {k: ref[k] for k in ('primal', 'dual', 'sign', 'gap')}
        bounds_of(case)
    return case


def bounds_of(case, scale=1.0):
    """E, tau and the vertex rows of a feasible case for the cost scale * c (the marginals scale with the cost, the minimiser does not)"""
    ref, c = case['ref'], case['c'] * scale
    C = max(1.0, np.abs(c).max())
    case['E'] = value_bound(c, np.concatenate([ref['y'], ref['z']]) * scale, case['nv'], case['m'])
    case['tau'] = 1e-3 * C
    case['rows'], case['nondegenerate'] = vertex_rows(dict(y=ref['y'] * scale), case['lp'][0], case['lp'][2], case['tau'])
    return case


def draw_cases(rng, per_combination=2):
    """every (counts, time) combination per_combination times, gradient kinds and table styles in rotation"""
    out, n = [], 0
    for counts in COUNTS:
        for time_how in TIMES:
            for r in range(per_combination):
                out.append(draw_case(rng, counts, time_how, GRADS[n % len(GRADS)], interleave=(n // len(GRADS)) % 2 == 1))
                n += 1
    return out
