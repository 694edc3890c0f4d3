"""What the tests of the torque-driven whole-body plant (test_wb_torque_plant_host.py, test_gpu_wb_torque_plant.py) share: a numpy restatement of
csrc/srbm_wb_fd.hiph -- the torque law, the constrained forward dynamics as one KKT system solved with np.linalg.solve, the sub-steps, the push
rule and ik_numpy.integrate -- built on wbc_numpy.Robot (dynamics_terms, foot_jacobian_lwa, foot_classical_acceleration) constructed with the
PLANT'S bodies, and the seeded inputs of the GPU tests, so that the host tests can check their conditioning without a GPU.  A plain module: no
fixtures, nothing pytest collects."""
import copy

import numpy as np

import controller_rollout_kit as kit
from controller_rollout_kit import ik, wbc

# contact patterns of the solve: none, each single foot, the two diagonals, two triples, all four (the stacking order is where it can go wrong)
PATTERNS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 0), (0, 1, 1, 1), (1, 1, 1, 1)]
# the robot's actuator gains of the tests (position / velocity actuators around the motors; NOT the QP's acceleration-level gains)
KP, KD = 20.0, 0.2


def plant_cfg(cfg, trunk_mass_factor=1.0, bodies=None):
    """cfg with the plant's bodies: the trunk heavier by a factor, or a body list of its own"""
    c = dict(cfg)
    c['body_model'] = copy.deepcopy(bodies if bodies is not None else cfg['body_model'])
    c['body_model'][0]['mass'] = c['body_model'][0]['mass'] * trunk_mass_factor
    return c


def perturbed_bodies(cfg, b):
    """bodies that differ from the controller's in every kind of entry, differently per instance b: masses, centres of mass, inertias"""
    bodies = copy.deepcopy(cfg['body_model'])
    for i, body in enumerate(bodies):
        body['mass'] = body['mass'] * (1.0 + 0.05 * (b + 1) + 0.01 * i)
        body['com'] = [c + 0.004 * (b + 1) * ((i + j) % 3 - 1) for j, c in enumerate(body['com'])]
        body['inertia'] = (np.asarray(body['inertia'], float) * (1.0 + 0.1 * (b + 1))).tolist()
    return bodies


def bodies_arrays(body_lists):
    """[batch] body lists -> mass[batch][13], com[batch][13][3], inertia[batch][13][3][3] (ControllerRollout.set_plant_bodies)"""
    return (np.array([[x['mass'] for x in bl] for bl in body_lists], float), np.array([[x['com'] for x in bl] for bl in body_lists], float),
            np.array([[np.asarray(x['inertia'], float).reshape(3, 3) for x in bl] for bl in body_lists], float))


def torque_law(control, q, v, kp, kd, lim, off=False):
    """-> tau[12], number of clamped joints, max |tau - tau_ff|.  control[36] = [q targets, v targets, feed-forward torques]; off: the tick returned
    a zero control action, the actuators are off"""
    control = np.asarray(control, float)
    tff = control[24:]
    if off:
        return np.zeros(12), 0, float(np.abs(tff).max())
    cmd = tff + kp * (control[:12] - q[7:]) + kd * (control[12:24] - v[6:])
    tau = np.minimum(np.maximum(cmd, -lim), lim)
    return tau, int(np.sum((cmd > lim) | (cmd < -lim))), float(np.abs(tau - tff).max())


def kkt_system(robot, q, v, tau, contact):
    """K x = r for x = (a[18], F stacked over the feet in contact in foot order): M a - Js' F = S' tau - C v - g, Js a = -Jsdot v"""
    idx = [i for i in range(4) if contact[i]]
    nc = len(idx)
    M, Cv, g = robot.dynamics_terms(q, v)
    Js = np.vstack([robot.foot_jacobian_lwa(q, i) for i in idx]) if nc else np.zeros((0, 18))
    gamma = np.concatenate([robot.foot_classical_acceleration(q, v, i) for i in idx]) if nc else np.zeros(0)
    n = 18 + 3 * nc
    K = np.zeros((n, n))
    K[:18, :18] = M; K[:18, 18:] = -Js.T; K[18:, :18] = Js
    r = np.concatenate([-(Cv + g), -gamma])
    r[6:18] += tau
    return K, r, Js, gamma


def forward_dynamics(robot, q, v, tau, contact):
    """-> sol[30]: (a, F) of the system above, zero past 18 + 3 nc"""
    K, r, _, _ = kkt_system(robot, q, v, tau, contact)
    sol = np.zeros(30)
    sol[:len(r)] = np.linalg.solve(K, r)
    return sol


def fd_step(robot, q, v, control, contact, off, kp, kd, lim, h, S, k, mass, Ir_inv, push=None):
    """tick k of the torque-driven plant for one instance: S sub-steps of h / S -> q+, v+, dict(pushed, clamped, deviation, sol, tau) of the last
    sub-step.  push: (time, impulse[6]) or None, applied after the last velocity update and before its configuration step"""
    q, v = np.array(q, float), np.array(v, float)
    hs = h / S
    pushed = push is not None and kit.push_applies(k * h, h, push[0])
    for s in range(S):
        tau, clamped, dev = torque_law(control, q, v, kp, kd, lim, off)
        sol = forward_dynamics(robot, q, v, tau, contact)
        hv = hs * sol[:18]
        v = v + hv
        if s == S - 1 and pushed:
            imp = np.asarray(push[1], float)
            v[:3] = v[:3] + imp[:3] / mass
            v[3:6] = v[3:6] + Ir_inv @ imp[3:]
        q = ik.integrate(q, v, hs)
    return q, v, dict(pushed=pushed, clamped=clamped, deviation=dev, sol=sol, tau=tau)


def quat_yaw_roll(yaw, roll):
    """xyzw of Rz(yaw) Rx(roll)"""
    qz = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]); qx = np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)])
    return ik.quat_mul(qz, qx)


def solve_cases(cfg, batch=4, seed=5):
    """the inputs of the solve-alone GPU test: a list of (q[batch][19], v[batch][18], tau[batch][12], contact[batch][4]) that covers every pattern
    of PATTERNS, joints 0.05 rad around init_config, bases yawed and rolled past 90 degrees, |tau| up to the torque bounds (some entries on them)"""
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    tb = np.asarray(cfg['torque_bounds'], float)
    pats = PATTERNS + [PATTERNS[5], PATTERNS[6]]
    calls = []
    for c in range(len(pats) // batch):
        q = np.tile(q0, (batch, 1)); q[:, 7:] += rng.uniform(-0.05, 0.05, size=(batch, 12))
        q[:, :3] += rng.normal(size=(batch, 3)) * 0.1
        for b in range(batch):
            yaw, roll = [(0.3, -0.2), (1.9, 0.1), (-2.6, 2.0), (0.7, -1.8)][(b + c) % 4]
            q[b, 3:7] = quat_yaw_roll(yaw, roll)
        v = rng.normal(size=(batch, 18)) * 0.5
        tau = rng.uniform(-1, 1, size=(batch, 12)) * tb
        tau[:, c] = tb[c]; tau[:, 11 - c] = -tb[11 - c]
        calls.append((q, v, tau, np.array(pats[batch * c:batch * (c + 1)], np.int32)))
    return calls


def step_cases(cfg, h, batch=4, seed=77):
    """the inputs of the plant-step GPU test, per round: dict(k, q, v, control, contact, status, push_time, impulse, want_push).  The QP statuses cover
    solved, reduced tolerances, iteration limit and failure (the last two: a zero control action); joint 4 of instance 1 is commanded beyond any limit
    the test sets"""
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    status = np.array([[0, 0 | 9 << 8], [1, 1 | 12 << 8], [0, 2 | 200 << 8], [2, 8]], np.int32)
    out = []
    for rnd, k in enumerate((0, 3, 41)):
        t_k = k * h
        q = np.tile(q0, (batch, 1)) + rng.normal(size=(batch, 19)) * 0.02
        q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
        v = rng.normal(size=(batch, 18)) * 0.3
        control = np.concatenate([q[:, 7:] + rng.normal(size=(batch, 12)) * 0.05, v[:, 6:] + rng.normal(size=(batch, 12)) * 0.2,
                                  rng.normal(size=(batch, 12)) * 5.0], axis=1)
        control[1, 24 + 4] = 60.0
        st = np.roll(status, rnd, axis=0)
        control[(st[:, 1] & 255) > 1] = 0.0                                  # what the tick returns with such a status
        contact = np.array([PATTERNS[6], PATTERNS[5], PATTERNS[9], PATTERNS[6]], np.int32)[np.roll(np.arange(batch), rnd)]
        out.append(dict(k=k, q=q, v=v, control=control, contact=contact, status=st,
                        push_time=np.array([t_k + h, t_k, t_k + 0.5 * h, -1.0]),   # fires at the end of the tick, not at its start, inside, never
                        impulse=rng.normal(size=(batch, 6)), want_push=np.array([True, False, True, False])))
    return out


def step_actuators(cfg, batch=4):
    """kp, kd, torque limits [batch][12] of the plant-step test: PD on, the configured torque bounds as limits but none on instance 3"""
    lim = np.tile(np.asarray(cfg['torque_bounds'], float), (batch, 1))
    lim[3] = np.inf
    return np.full((batch, 12), KP), np.full((batch, 12), KD), lim
