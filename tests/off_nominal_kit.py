"""The off-nominal cases of the whole-body QP and of the inverse kinematics, with their references (test_off_nominal_host.py checks the conditions on
them, test_gpu_off_nominal.py holds the kernels to them).  A plain module: no fixtures, nothing pytest collects.  Seeded, numpy only (the
certificate of qp_polish uses scipy's non-negative least squares); every family and every reference is computed once and shared: treat what
these functions return as read-only.

    PATTERNS, QP_FAMILIES, qp_family       16 whole-body QPs per family, one per contact pattern
    qp_reference                           build_qp -> cone form of wbc.solve_qp -> qp_solve at 1e-12 -> qp_polish.polish, the torques, the tight rows
    qp_data_response, qp_data_bounds       rounding floor of A, lb, ub, P, w and the bounds of the GPU comparison made from it
    IK_FAMILIES, ik_family, ik_reference   (state13, ee_des, q_guess) cases, ik.inverse_kinematics on them
    ik_instrumented                        a copy of that loop that also returns the deciding error norms and the number of large joint steps
    ik_response, ik_bound                  rounding floor of q over the cases that converge on all feet, and the bound made from it
    response                               largest change of a function's outputs under rounding-sized perturbations of its inputs"""
import functools
import os
import sys

import numpy as np

from oracle_py import load_config, qp_solve
from qp_polish import polish

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ik_numpy as ik
import wbc_numpy as wbc

PATTERNS = [[(p >> i) & 1 for i in range(4)] for p in range(16)]
QP_FAMILIES = ('saturated', 'friction', 'grf', 'tumbling')
QP_SEEDS = dict(saturated=101, friction=102, grf=103, tumbling=104)         # case c of a family is drawn from default_rng([seed, c, draw of that case])
# The velocity noise of 0.1 m/s asks the torso task for base accelerations of 300 m/s^2 (base_pos_gains), so whether the feet of a `grf` case are pushed to
# zero force or to force_bound is the sign of that noise: these cases take a later draw, the first one at which a foot in contact ends at zero force
GRF_DRAWS = {5: 1, 6: 2, 7: 1, 9: 3, 12: 1, 13: 4, 14: 1}
IK_FAMILIES = ('mid', 'reach')
# case c of a family is drawn from default_rng([seed, c]).  Scanned from 201 / 301 upwards: the first `mid` seed with four cases that converge on all feet
# after joint steps above SMALL_STEP, the first `reach` seed at which more than half of the cases converge on all feet (a leg at 0.98 of its reach is next to
# the singularity of the straight knee; most draws leave a foot at IT_MAX)
IK_SEEDS = dict(mid=208, reach=304)
IK_MID_DISTANCES = (0.05, 0.10, 0.10, 0.15)          # three cases each
SMALL_STEP = 0.125                                   # SRBM_IK_SMALL_ANGLE: above it the kernel takes sin / cos from the library routine
TIGHT = 1e-9
MARGIN = 1000.0                                      # allowance for a different but equally plain order of a few hundred operations
DATA_CAPS = dict(A=1e-9, lb=1e-8, ub=1e-8, P=1e-12, w=1e-8)      # no bound above those of test_gpu_wbc.py
IK_CAP = 1e-10


def response(fn, inputs, seed=7, relative=False, base=None):
    """fn(*inputs) -> dict of arrays.  The largest change of every output over three seeded perturbations of every entry of every input by a relative
    2^-50 (sign drawn per entry): the rounding floor of fn on these inputs.  relative: per output, divided by max(1, |output|_inf).  base: fn(*inputs),
    where the caller has it already."""
    rng = np.random.default_rng(seed)
    inputs = [np.asarray(a, float) for a in inputs]
    base = fn(*inputs) if base is None else base
    out = {k: 0.0 for k in base}
    for trial in range(3):
        moved = fn(*[a * (1.0 + rng.choice([-1.0, 1.0], size=a.shape) * 2.0 ** -50) for a in inputs])
        for k in base:
            a, b = np.asarray(base[k], float), np.asarray(moved[k], float)
            if a.size:
                out[k] = max(out[k], np.abs(a - b).max() / (max(1.0, np.abs(a).max()) if relative else 1.0))
    return out


# ---------------------------------------------------------------- whole-body QP ----------------------------------------------------------------
@functools.lru_cache(None)
def world():
    cfg = load_config()
    return cfg, wbc.Robot(cfg), np.array(cfg['init_config'], float), np.array(cfg['leg_origins'], float)


def _axis(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def _qp_case(name, case, pattern, rng):
    cfg, robot, q0, legs = world()
    nc, mg = sum(pattern), cfg['mass'] * wbc.GRAV
    q, q_des, v_des = q0.copy(), q0.copy(), np.zeros(18)
    q[7:] += rng.normal(size=12) * 0.1
    v = rng.normal(size=18) * 0.1
    f = np.tile([0.0, 0.0, mg / max(nc, 1)], (nc, 1))
    if name == 'saturated':
        q_des[7:] += rng.choice([-1.0, 1.0], 12) * rng.uniform(0.3, 0.8, 12)
    elif name == 'friction':
        for i in range(nc):
            sx, sy = rng.choice([-1.0, 1.0], 2)
            f[i] = [sx * rng.uniform(0.8, 2.0) * mg / nc, sy * rng.uniform(0.0, 2.0) * mg / nc, mg / nc]
    elif name == 'grf':
        for i in range(nc):
            f[i] = [rng.normal() * 5.0, rng.normal() * 5.0, -0.5 * mg if i % 2 == 0 else 2.0 * cfg['force_bound']]
    elif name == 'tumbling':
        angle = rng.uniform(0.2, 2.2)
        quat = wbc.exp3_quat(angle * _axis(rng))
        q[3:7] = -quat if case % 3 == 0 else quat                                  # every third one as the other representative (w < 0)
        q[7:] = q0[7:] + rng.normal(size=12) * 0.4
        q[:3] = q0[:3] + rng.normal(size=3) * 0.1
        v = rng.normal(size=18) * np.concatenate([np.full(3, 1.0), np.full(3, 2.0), np.full(12, 6.0)])
        q_des[7:] += rng.normal(size=12) * 0.3
        q_des[3:7] = wbc.exp3_quat(0.3 * _axis(rng))
        v_des = rng.normal(size=18) * 0.5
        for i in range(nc):
            f[i] = [rng.normal() * mg / nc, rng.normal() * mg / nc, rng.uniform(-0.3, 1.5) * mg / nc]
    else:
        raise KeyError(name)
    fdes = np.zeros(12)
    fdes[:3 * nc] = f.reshape(-1)
    return q, v, q_des, v_des, fdes


@functools.lru_cache(None)
def qp_family(name):
    """dict(q [16][19], v [16][18], contact [16][4] int32, q_des, v_des, fdes [16][12]: the targets of the feet in contact stacked, zero behind them)"""
    rows = [_qp_case(name, c, PATTERNS[c], np.random.default_rng([QP_SEEDS[name], c, GRF_DRAWS.get(c, 0) if name == 'grf' else 0])) for c in range(16)]
    out = {k: np.array([r[i] for r in rows]) for i, k in enumerate(('q', 'v', 'q_des', 'v_des', 'fdes'))}
    out['contact'] = np.array(PATTERNS, np.int32)
    return out


def negated_base_quaternion(fam):
    """the same family with every base quaternion as its other representative"""
    out = dict(fam)
    out['q'] = fam['q'].copy()
    out['q'][:, 3:7] *= -1.0
    return out


def base_rotation_angle(quat):
    return 2.0 * np.arctan2(np.linalg.norm(quat[:3]), abs(quat[3]))


def cone_form(A, lb, ub):
    """wbc.solve_qp's conversion: equality rows as the zero cone, then every finite upper bound, then every finite lower bound as non-negative rows
    (test_off_nominal_host.py holds the interior-point minimiser of qp_reference to wbc.solve_qp's, bit for bit)"""
    eq = lb == ub
    up, lo = (~eq) & (ub < wbc.INF / 2), (~eq) & (lb > -wbc.INF / 2)
    Ac, bc = np.vstack([A[eq], A[up], -A[lo]]), np.concatenate([ub[eq], ub[up], -lb[lo]])
    is_eq = np.zeros(len(bc), bool)
    is_eq[:eq.sum()] = True
    return Ac, bc, is_eq, [(0, int(eq.sum())), (1, int(up.sum() + lo.sum()))]


def _build(fam, b):
    cfg, robot, q0, legs = world()
    nc = int(fam['contact'][b].sum())
    return wbc.build_qp(robot, cfg, fam['q'][b], fam['v'][b], fam['contact'][b], fam['q_des'][b], fam['v_des'][b], fam['fdes'][b, :3 * nc])


@functools.lru_cache(None)
def qp_reference(name, negate=False):
    """per case: dict(nc, n, m, A, lb, ub, P (diagonal), w, status, iters, x_ipm, x (the polished, certified minimiser, None without certificate),
    info, tau (torques of x by the formula of wbc.control_action), torque_tight, pyramid_tight (numbers of tight rows), fz (per foot in contact))"""
    cfg, robot, q0, legs = world()
    fam = negated_base_quaternion(qp_family(name)) if negate else qp_family(name)
    out = []
    for b in range(16):
        nc = int(fam['contact'][b].sum())
        A, lb, ub, P, w, (M, Cv, g, Js) = _build(fam, b)
        Ac, bc, is_eq, cones = cone_form(A, lb, ub)
        r = qp_solve(P, w, Ac, bc, cones, tol_gap=1e-12, tol_feas=1e-12)
        x, info = polish(P, w, Ac, bc, is_eq, r['x'], r['z'], r['s'])
        rec = dict(nc=nc, n=18 + 3 * nc, m=6 + 7 * nc + 12 + nc, A=A, lb=lb, ub=ub, P=np.diag(P).copy(), w=w, status=r['status'], iters=r['iters'],
                   x_ipm=r['x'], x=x, info=info)
        if x is not None:
            Ax, r0 = A @ x, 6 + 3 * nc
            hi, lo = (ub - Ax < TIGHT) & (lb != ub), (Ax - lb < TIGHT) & (lb != ub)
            rec['tau'] = (M @ x[:18] - Js.T @ x[18:] + Cv + g)[6:]
            rec['torque_tight'] = int((hi | lo)[r0:r0 + 12].sum())
            rec['pyramid_tight'] = int(hi[r0 + 12:r0 + 12 + 4 * nc].sum())
            rec['tight'] = int((hi | lo).sum())
            rec['fz'] = x[18:].reshape(nc, 3)[:, 2].copy()
        out.append(rec)
    return out


def _data_fn(contact):
    cfg, robot, q0, legs = world()

    def fn(q, v, q_des, v_des, f):
        A, lb, ub, P, w, _ = wbc.build_qp(robot, cfg, q, v, contact, q_des, v_des, f)
        return dict(A=A, lb=lb[np.abs(lb) < 1e29], ub=ub, P=np.diag(P), w=w)
    return fn


@functools.lru_cache(None)
def qp_data_response(name):
    """{A, lb, ub, P, w: the largest response of build_qp over the family's 16 cases, relative to max(1, |.|_inf)}"""
    fam = qp_family(name)
    worst = dict(A=0.0, lb=0.0, ub=0.0, P=0.0, w=0.0)
    for b in range(16):
        nc = int(fam['contact'][b].sum())
        r = response(_data_fn(fam['contact'][b]), [fam['q'][b], fam['v'][b], fam['q_des'][b], fam['v_des'][b], fam['fdes'][b, :3 * nc]],
                     seed=1000 + b, relative=True)
        worst = {k: max(worst[k], r[k]) for k in worst}
    return worst


@functools.lru_cache(None)
def qp_data_bounds():
    """per quantity: MARGIN x the largest response over the four families, and never above the bound test_gpu_wbc.py uses"""
    return {k: min(MARGIN * max(qp_data_response(f)[k] for f in QP_FAMILIES), DATA_CAPS[k]) for k in DATA_CAPS}


# ---------------------------------------------------------------- inverse kinematics ----------------------------------------------------------------
def _ik_pose(rng, roll, joints):
    cfg, robot, q0, legs = world()
    q = q0.copy()
    q[7:] += rng.normal(size=12) * joints
    q[3:7] = wbc.exp3_quat(rng.normal(size=3) * roll)
    state = np.zeros(13)
    state[:3] = q[:3] + rng.normal(size=3) * 0.01
    state[6:10] = q[3:7]
    return q, state


@functools.lru_cache(None)
def ik_family(name):
    """dict(state [C][13], ee_des [C][4][3], q_guess [C][19]): 12 `mid` cases (targets 0.05 / 0.10 / 0.10 / 0.15 m, three cases each, in random directions
    from the feet of a pose with joints + N(0, 0.3) and the base rolled by N(0, 0.3 .. 0.5) rad) or 6 `reach` cases (targets on the hip-to-foot ray at
    0.98 of the two link lengths, from a pose with joints + N(0, 0.2) and the base rolled by N(0, 0.3) rad); the guess is the nominal configuration"""
    cfg, robot, q0, legs = world()
    states, dess = [], []
    for c in range(12 if name == 'mid' else 6):
        rng = np.random.default_rng([IK_SEEDS[name], c])
        q, state = _ik_pose(rng, (0.3, 0.4, 0.5)[c % 3], 0.3) if name == 'mid' else _ik_pose(rng, 0.3, 0.2)
        ee = ik.forward_kinematics(legs, q)
        if name == 'mid':
            u = rng.normal(size=(4, 3))
            des = ee + IK_MID_DISTANCES[c // 3] * u / np.linalg.norm(u, axis=1, keepdims=True)
        else:
            Rb, des = ik.quat_to_R(q[3:7]), ee.copy()
            for e in range(4):
                hip = q[:3] + Rb @ (legs[e][0] + legs[e][1])
                des[e] = hip + 0.98 * (np.linalg.norm(legs[e][2]) + np.linalg.norm(legs[e][3])) * (ee[e] - hip) / np.linalg.norm(ee[e] - hip)
        states.append(state); dess.append(des)
    return dict(state=np.array(states), ee_des=np.array(dess), q_guess=np.tile(q0, (len(states), 1)))


def ik_cases():
    """the 18 cases in one batch, `mid` first"""
    fams = [ik_family(f) for f in IK_FAMILIES]
    return {k: np.concatenate([f[k] for f in fams]) for k in fams[0]}


@functools.lru_cache(None)
def ik_reference():
    """ik.inverse_kinematics on the 18 cases: list of (q, iterations per foot, ok)"""
    legs, c = world()[3], ik_cases()
    return [ik.inverse_kinematics(legs, c['state'][b], c['ee_des'][b], c['q_guess'][b]) for b in range(len(c['state']))]


def ik_converged_cases():
    return [b for b, (q, it, ok) in enumerate(ik_reference()) if max(it) < ik.IT_MAX]


def ik_instrumented(legs, state13, ee_des, q_guess):
    """ik.inverse_kinematics, statement by statement, that also returns per foot (error norm of the last iteration, error norm of the one before it
    or None, number of iterations whose joint step exceeds SMALL_STEP).  Serves the conditions of test_off_nominal_host.py only (which also holds
    its q and iteration counts to ik.inverse_kinematics bit for bit)."""
    q = np.array(q_guess, float).copy()
    q[:3] = state13[:3]; q[3:7] = state13[6:10]
    R_des, p_des = ik.quat_to_R(state13[6:10]), np.asarray(state13[:3], float)
    iters, feet = [], []
    for ee in range(4):
        it, last, prev, big = 0, None, None, 0
        for it in range(ik.IT_MAX):
            q[3:7] = ik.first_order_normalize(q[3:7])
            err, J = ik.ik_error_and_jacobian(legs, q, ee, p_des, R_des, np.asarray(ee_des[ee], float))
            prev, last = last, np.linalg.norm(err)
            if last < ik.EPS:
                break
            v = -(J.T @ np.linalg.solve(J @ J.T + ik.DAMP * np.eye(9), err))
            big += int(np.abs(ik.DT * v[6:]).max() > SMALL_STEP)
            q = ik.integrate(q, v, ik.DT)
        else:
            it = ik.IT_MAX
        iters.append(it); feet.append((last, prev, big))
    return q, iters, feet


@functools.lru_cache(None)
def ik_response():
    """per case that converges on all feet: the response of q (absolute, q is of order one) and whether the iteration counts moved"""
    legs, c, ref = world()[3], ik_cases(), ik_reference()
    out = {}
    for b in ik_converged_cases():
        moved = []

        def fn(state, des):
            q, it, ok = ik.inverse_kinematics(legs, state, des, c['q_guess'][b])
            moved.append(list(it) != list(ref[b][1]))
            return dict(q=q)
        out[b] = (response(fn, [c['state'][b], c['ee_des'][b]], seed=2000 + b, base=dict(q=ref[b][0]))['q'], any(moved))
    return out


def ik_bound():
    return min(MARGIN * max(r for r, moved in ik_response().values()), IK_CAP)
