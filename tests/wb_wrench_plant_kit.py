"""What the tests of the torque-driven plant's wrench schedule (test_wb_wrench_plant_host.py, test_gpu_wb_wrench_plant.py) share, built on the
restatements of wb_torque_plant_kit.py, wb_ground_plant_kit.py, wb_terrain_plant_kit.py and wb_joint_plant_kit.py: the activity rule of
include/srbm_rti.h ("timed external wrenches") in np.float64, operation by operation; the body poses from wbc_numpy.Robot.joint_transforms and
ik_numpy; the generalized force Q from an analytic Jacobian of its own (Jv' F + Jw' N, not the device's column formulas); the wrench as a wrapper
of the plant's model whose g carries -Q, so that the restated solves take it unchanged; the step on the three surfaces with and without a joint
model; the record; and the seeded schedules of the GPU tests.  A plain module: no fixtures, nothing pytest collects."""
import numpy as np

import controller_rollout_kit as kit
import wb_joint_plant_kit as jk
import wb_torque_plant_kit as fd
from controller_rollout_kit import ik

INF = float('inf')
EVENTS, EVENT_DOUBLES = 8, 16
WT0, WD, WBODY, WFRAME = 0, 1, 2, 3
WORLD, BODY = 0, 1
HELD, GROUND, TERRAIN = jk.HELD, jk.GROUND, jk.TERRAIN
f64 = np.float64


def event(t0, d, body, r=(0, 0, 0), force=(0, 0, 0), torque=(0, 0, 0), frame=WORLD):
    e = np.zeros(EVENT_DOUBLES)
    e[0], e[1], e[2], e[3], e[4:7], e[7:10], e[10:13] = t0, d, body, frame, r, force, torque
    return e


def pad(events, n=None):
    """a list of events -> [n][16] with empty slots (d = 0) behind them"""
    n = max(1, len(events)) if n is None else n
    out = np.zeros((n, EVENT_DOUBLES))
    for i, e in enumerate(events):
        out[i] = e
    return out


# ---- the activity rule ----
def substep_time(tick, h, S, s):
    """ts of sub-step s of tick `tick`: every line one rounded operation"""
    h = f64(h)
    hs = h / f64(S)
    tk = f64(tick) * h
    p = f64(s) * hs
    return tk + p


def active(w, ts):
    t0, d = f64(w[WT0]), f64(w[WD])
    with np.errstate(invalid='ignore'):
        te = t0 + d
    return bool(d != 0.0 and ts >= t0 and ts < te)


def active_mask(W, ts):
    """W[n][16] of one instance -> the mask of its events active at ts"""
    return sum(1 << e for e, w in enumerate(W) if active(w, ts))


def active_masks(W, first_tick, ticks, h, S):
    """W[batch][n][16] -> mask[ticks][S][batch]"""
    out = np.zeros((ticks, S, len(W)), np.int32)
    for k in range(ticks):
        for s in range(S):
            ts = substep_time(first_tick + k, h, S, s)
            for b in range(len(W)):
                out[k, s, b] = active_mask(W[b], ts)
    return out


# ---- the body poses and the generalized force ----
def body_pose(robot, q, body):
    """-> R (world from body), origin (world) of body 0..12 through the chain of joint_transforms: child = E parent, the joint at r in the parent"""
    R, o = ik.quat_to_R(q[3:7]), np.array(q[:3], float)
    if body == 0:
        return R, o
    ee, k = (body - 1) // 3, (body - 1) % 3
    JT = robot.joint_transforms(q)
    for j in range(k + 1):
        E = JT[ee][j][0][:3, :3]
        o = o + R @ robot.legs[ee][j]
        R = R @ E.T
    return R, o


def point_jacobians(robot, q, body, r):
    """-> x, Jv[3][18], Jw[3][18]: d(world point)/dt = Jv v, world angular velocity of the body = Jw v, for the point at r in the body's frame"""
    Rb, pb = ik.quat_to_R(q[3:7]), np.array(q[:3], float)
    R, o = body_pose(robot, q, body)
    x = o + R @ np.asarray(r, float)
    Jv, Jw = np.zeros((3, 18)), np.zeros((3, 18))
    Jv[:, :3] = Rb
    Jv[:, 3:6] = -ik.skew(x - pb) @ Rb
    Jw[:, 3:6] = Rb
    if body > 0:
        ee, k = (body - 1) // 3, (body - 1) % 3
        for j in range(k + 1):
            Rj, cj = body_pose(robot, q, 1 + 3 * ee + j)
            a = Rj[:, 0 if j == 0 else 1]           # the joint's axis is fixed in its own body: x for the hip, y for thigh and calf
            Jv[:, 6 + 3 * ee + j] = np.cross(a, x - cj)
            Jw[:, 6 + 3 * ee + j] = a
    return x, Jv, Jw


def world_wrench(robot, q, w):
    R, _ = body_pose(robot, q, int(w[WBODY]))
    F, N = np.array(w[7:10], float), np.array(w[10:13], float)
    if w[WFRAME] != 0:
        F, N = R @ F, R @ N
    return F, N


def generalized_force(robot, q, W, mask):
    """Q[18] of the events of `mask` among W[n][16], and the sum of their world forces"""
    Q, Fsum = np.zeros(18), np.zeros(3)
    for e, w in enumerate(W):
        if mask >> e & 1:
            F, N = world_wrench(robot, q, w)
            _, Jv, Jw = point_jacobians(robot, q, int(w[WBODY]), w[4:7])
            Q = Q + Jv.T @ F + Jw.T @ N
            Fsum = Fsum + F
    return Q, Fsum


# ---- the wrench in the solves: a model whose g carries -Q (every restated solve forms its right-hand side as tau - C v - g) ----
class _WrenchRobot:
    def __init__(self, robot, Q):
        self._robot, self._Q = robot, Q

    def __getattr__(self, name):
        return getattr(self._robot, name)

    def dynamics_terms(self, q, v):
        M, Cv, g = self._robot.dynamics_terms(q, v)
        return M, Cv, g - self._Q


class WithWrench:
    def __init__(self, model, Q):
        self._model = model
        self.robot = _WrenchRobot(model.robot, Q)

    def __getattr__(self, name):
        return getattr(self._model, name)


def record_fold(rec, S, hs, history):
    """history: per sub-step (mask, |Q|_inf, sum of the world forces) -> the record after"""
    rec = np.array(rec, float)
    rec[0] += S
    for mask, qinf, Fsum in history:
        if mask:
            rec[1] += 1
            rec[2] = float(int(rec[2]) | mask)
            rec[3] = max(rec[3], qinf)
            rec[4:7] += hs * Fsum
    return rec


def wrench_step(surface, model, q, v, control, off, kp, kd, lim, W, h, S, k, mass, Ir_inv, push=None, contact=None, cs=None, gr=None, terrain=None,
                J=None, stops=None, js=None):
    """tick k of the torque-driven plant with the schedule W[n][16] for one instance, with a joint model (J, stops, js) or without (J None):
    -> q+, v+, cs+ (None with the feet held), js+ (None without a joint model), dict(pushed, sol, history: per sub-step (mask, |Q|_inf, F sum))"""
    q, v = np.array(q, float), np.array(v, float)
    cs = None if cs is None else np.array(cs, float).reshape(4, 3)
    js = None if J is None else np.array(js, float)
    Jm = jk.transparent() if J is None else np.asarray(J, float)
    hs = h / S
    pushed = push is not None and kit.push_applies(k * h, h, push[0])
    history = []
    for s in range(S):
        tau, _, _ = fd.torque_law(control, q, v, kp, kd, lim, off)
        if J is not None:
            tau, js, _ = jk.law_substep(Jm, stops, hs, tau, q[7:], v[6:], js)
        mask = active_mask(W, substep_time(k, h, S, s))
        m = model
        if mask:
            Q, Fsum = generalized_force(model.robot, q, W, mask)
            m = WithWrench(model, Q)
            history.append((mask, float(np.abs(Q).max()), Fsum))
        else:
            history.append((0, 0.0, np.zeros(3)))
        sol, cs_new, _ = jk.dynamics(surface, m, Jm, q, v, tau, contact, cs, gr, terrain)
        if surface != HELD:
            cs = cs_new
        hv = hs * sol[:18]
        v = v + hv
        if s == S - 1 and pushed:
            imp = np.asarray(push[1], float)
            v[:3] = v[:3] + imp[:3] / mass
            v[3:6] = v[3:6] + Ir_inv @ imp[3:]
        q = ik.integrate(q, v, hs)
    return q, v, cs, js, dict(pushed=pushed, sol=sol, history=history)


# ---- the inputs of the tests ----
def force_cases(cfg, seed=91):
    """26 instances, one per (body, frame): a random posture, an off-origin point, a force and a torque; the event is active at `time`, and a second
    event of the instance is not -> dict(q[26][19], W[26][2][16], time[26])"""
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    n = 26
    q = np.tile(q0, (n, 1))
    q[:, :3] += rng.normal(size=(n, 3)) * 0.2
    q[:, 7:] += rng.uniform(-0.4, 0.4, (n, 12))
    quat = rng.normal(size=(n, 4))
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    W = np.zeros((n, 2, EVENT_DOUBLES))
    time = rng.uniform(0.1, 1.0, n)
    for i in range(n):
        body, frame = i // 2, i % 2
        W[i, 0] = event(time[i] - 0.01, 0.02, body, rng.uniform(-0.15, 0.15, 3), rng.uniform(-40, 40, 3), rng.uniform(-5, 5, 3), frame)
        W[i, 1] = event(time[i] + 0.5, 0.1, (body + 5) % 13, rng.uniform(-0.1, 0.1, 3), rng.uniform(-40, 40, 3), rng.uniform(-5, 5, 3), 1 - frame)
    return dict(q=q, W=W, time=time)


STEP_TICKS = (0, 3, 41)          # the ticks of the step cases of the three plant kits


def step_schedule(k, h, S, batch=4, seed=93):
    """the schedules of the step test for tick k -> W[batch][3][16]: per instance events on three different bodies, event 1 in the body frame.
    S > 1: event 0 starts strictly between the times of sub-steps 1 and 2 and stays on, event 1 is on from before the tick and ends strictly
    between sub-steps 0 and 1, event 2 starts between sub-steps 2 and 3 (even instances) or lies wholly between two sub-step times and never acts
    (odd ones): sub-step 0 has event 1, sub-step 1 none, sub-step 2 event 0, sub-step 3 events 0 and 2.
    S == 1: times on the rollout's clock -- event 0 is on in tick 3 alone, event 1 from tick 41 on, event 2 (odd instances) ends before tick 3 begins
    and starts after tick 0 -- so tick 0 has no event and the other ticks of STEP_TICKS have one"""
    rng = np.random.default_rng(seed + k)
    hs, tk = h / S, k * h
    W = np.zeros((batch, 3, EVENT_DOUBLES))
    for b in range(batch):
        bodies = rng.permutation(13)[:3]
        wr = lambda i, fr: dict(body=int(bodies[i]), r=rng.uniform(-0.1, 0.1, 3), force=rng.uniform(-30, 30, 3), torque=rng.uniform(-3, 3, 3), frame=fr)
        if S == 1:
            W[b, 0] = event(2.5 * h, 1.2 * h, **wr(0, WORLD))
            W[b, 1] = event(40.5 * h, INF, **wr(1, BODY))
            W[b, 2] = event(0.5 * h, 1.7 * h, **wr(2, BODY)) if b % 2 else np.zeros(EVENT_DOUBLES)
        else:
            W[b, 0] = event(tk + 1.4 * hs, INF, **wr(0, WORLD))
            W[b, 1] = event(tk - 0.4 * hs, 0.9 * hs, **wr(1, BODY))
            W[b, 2] = event(tk + 2.3 * hs, 0.4 * hs, **wr(2, WORLD)) if b % 2 else event(tk + 2.6 * hs, 5 * h, **wr(2, BODY))
    return W
