"""What the tests of the torque-driven plant's ground (test_wb_ground_plant_host.py, test_gpu_wb_ground_plant.py) share: a numpy restatement of
csrc/srbm_wb_ground.hiph -- the contact law per foot, the unconstrained 18-row solve with the ground forces on the right-hand side, the sub-steps
with the contact state carried along, the push rule -- built on wbc_numpy.Robot (dynamics_terms, foot_jacobian_lwa) constructed with the PLANT'S
bodies and ik_numpy.forward_kinematics, with the torque law of wb_torque_plant_kit; the seeded inputs of the GPU tests, so that the host tests can
check their branch margins without a GPU; and the drop-and-settle case with its thresholds.  A plain module: no fixtures, nothing pytest collects."""
import numpy as np

import controller_rollout_kit as kit
import wb_torque_plant_kit as fd
from controller_rollout_kit import ik

NO_CONTACT = np.zeros((4, 3))
# the branches of the contact law a foot can take
AIR, STICK, SLIP, CLAMP = 'air', 'stick', 'slip', 'clamp'          # clamp: penetrating, but rebounding so fast that N is clamped to 0


def ground_params(z0, k_n=4000.0, d_n=60.0, mu=0.6, k_t=3000.0, d_t=30.0):
    return np.array([z0, k_n, d_n, mu, k_t, d_t, 0.0, 0.0])


def contact_law(p, w, cs, gr):
    """foot position p[3], velocity w[3], state cs = (in_contact, anchor_x, anchor_y), ground gr[8] -> F[3], new cs[3], info: the branch, whether
    it is a first touch, and the margins of the decisions taken (delta; the unclamped normal force; n0 - lim relative to max(1, lim))"""
    z0, k_n, d_n, mu, k_t, d_t = gr[:6]
    delta = z0 - p[2]
    if not delta > 0:
        return np.zeros(3), np.zeros(3), dict(branch=AIR, first=False, slip=False, margins=[abs(delta)])
    first = not cs[0]
    anchor = np.array(p[:2], float) if first else np.array(cs[1:3], float)
    n1 = k_n * delta - d_n * w[2]
    N = max(0.0, n1)
    dw = d_t * w[:2]
    T0 = -(k_t * (p[:2] - anchor)) - dw
    lim = mu * N
    n0 = np.sqrt(T0[0] * T0[0] + T0[1] * T0[1])
    if n0 <= lim:
        T, slip = T0, False
    else:
        T = (lim / n0) * T0
        anchor = p[:2] + (T + dw) / k_t
        slip = True
    info = dict(branch=CLAMP if not n1 > 0 else (SLIP if slip else STICK), first=first, slip=slip,
                margins=[abs(delta), abs(n1), abs(n0 - lim) / max(1.0, lim)], N=N, T0=T0, lim=lim)
    return np.array([T[0], T[1], N]), np.array([1.0, anchor[0], anchor[1]]), info


def ground_dynamics(model, q, v, tau, cs, gr):
    """the law on the four feet and M a = S' tau - C v - g + sum_i J_i' F_i -> sol[30] = (a, F[4][3]), cs_out[4][3], the four infos of the law"""
    robot = model.robot
    p = ik.forward_kinematics(model.legs, q)
    J = [robot.foot_jacobian_lwa(q, i) for i in range(4)]
    F, out, infos = np.zeros((4, 3)), np.zeros((4, 3)), []
    for i in range(4):
        F[i], out[i], info = contact_law(p[i], J[i] @ v, np.asarray(cs, float).reshape(4, 3)[i], gr)
        infos.append(info)
    M, Cv, g = robot.dynamics_terms(q, v)
    r = -(Cv + g)
    r[6:] += tau
    for i in range(4):
        r = r + J[i].T @ F[i]
    return np.concatenate([np.linalg.solve(M, r), F.reshape(12)]), out, infos


def ground_step(model, q, v, cs, control, off, kp, kd, lim, gr, h, S, k, mass, Ir_inv, push=None):
    """tick k of the plant on its ground for one instance: S sub-steps of h / S -> q+, v+, cs+, dict(pushed, clamped, deviation, sol, tau, infos)
    of the last sub-step and `history`, the infos of every sub-step.  push as in wb_torque_plant_kit.fd_step"""
    q, v, cs = np.array(q, float), np.array(v, float), np.array(cs, float).reshape(4, 3)
    hs = h / S
    pushed = push is not None and kit.push_applies(k * h, h, push[0])
    history = []
    for s in range(S):
        tau, clamped, dev = fd.torque_law(control, q, v, kp, kd, lim, off)
        sol, cs, infos = ground_dynamics(model, q, v, tau, cs, gr)
        history.append(infos)
        hv = hs * sol[:18]
        v = v + hv
        if s == S - 1 and pushed:
            imp = np.asarray(push[1], float)
            v[:3] = v[:3] + imp[:3] / mass
            v[3:6] = v[3:6] + Ir_inv @ imp[3:]
        q = ik.integrate(q, v, hs)
    return q, v, cs, dict(pushed=pushed, clamped=clamped, deviation=dev, sol=sol, tau=tau, infos=infos, history=history)


def ground_word(cs, infos, plan):
    """the word of tick log field 63 (without its offset of 4096) from the contact state and the law's infos of the last sub-step and the plan's flags"""
    word = 0
    for i in range(4):
        inc = bool(cs[i][0])
        word |= int(inc) << i | int(inc and infos[i]['slip']) << (4 + i) | int(bool(plan[i]) != inc) << (8 + i)
    return word


def set_foot_velocity(model, q, v, foot, w):
    """v with the joint velocities of leg `foot` changed so that the foot moves with world velocity w (the base twist stays)"""
    J = model.robot.foot_jacobian_lwa(q, foot)
    c = slice(6 + 3 * foot, 9 + 3 * foot)
    v = np.array(v, float)
    v[c] = np.linalg.solve(J[:, c], np.asarray(w, float) - J[:, :6] @ v[:6])
    return v


# ---- the inputs of the law-and-solve GPU test ----
# per call and instance: the branches wanted on the feet that penetrate, from the deepest up, (branch, first touch); the feet above z0 are in the air
SOLVE_BRANCHES = [[((STICK, False), (SLIP, False), (CLAMP, False)), ((SLIP, True), (STICK, True), (CLAMP, True)),
                   ((CLAMP, False), (STICK, True), (SLIP, False)), ((SLIP, False), (SLIP, True), (STICK, False))],
                  [((STICK, False), (SLIP, True)), ((CLAMP, True), (STICK, False), (STICK, True)),
                   ((SLIP, False),), ((STICK, True), (CLAMP, False), (SLIP, True))]]


def solve_cases(cfg, models, batch=4, seed=11):
    """-> a list of dict(q, v, tau, cs, ground, want): want[b][foot] = (branch, first touch).  Bases yawed and rolled, z0 between two foot heights so
    that the feet of one instance sit in different branches; the foot velocities and the old anchors are set so that every foot takes the branch
    SOLVE_BRANCHES names with a wide margin (asserted on the restatement by the host test).  models[b]: the plant's model of instance b"""
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    tb = np.asarray(cfg['torque_bounds'], float)
    calls = []
    for c, branches in enumerate(SOLVE_BRANCHES):
        q = np.tile(q0, (batch, 1)); q[:, 7:] += rng.uniform(-0.05, 0.05, size=(batch, 12))
        q[:, :3] += rng.normal(size=(batch, 3)) * 0.1
        v = rng.normal(size=(batch, 18)) * 0.3
        tau = rng.uniform(-1, 1, size=(batch, 12)) * tb
        cs, ground, want = np.zeros((batch, 4, 3)), np.zeros((batch, 8)), []
        for b in range(batch):
            yaw, roll = [(0.3, -0.2), (1.9, 0.15), (-2.6, 0.3), (0.7, -0.25)][(b + c) % 4]
            q[b, 3:7] = fd.quat_yaw_roll(yaw, roll)
            p = ik.forward_kinematics(models[b].legs, q[b])
            order = np.argsort(p[:, 2])                        # the feet from the lowest up
            n = len(branches[b])
            z0 = 0.5 * (p[order[n - 1], 2] + p[order[n], 2]) if n < 4 else p[order[3], 2] + 0.01
            gr = ground_params(z0, k_n=3000.0 + 500.0 * b, d_n=40.0 + 10.0 * b, mu=0.5 + 0.1 * b, k_t=2500.0 + 300.0 * b, d_t=25.0 + 5.0 * b)
            wanted = [(AIR, False)] * 4
            for rank, (branch, first) in enumerate(branches[b]):
                i = int(order[rank])
                wanted[i] = (branch, first)
                delta = z0 - p[i, 2]
                spring = gr[1] * delta
                along = rng.normal(size=2); along /= np.linalg.norm(along)
                if branch == CLAMP:                            # rebounding: d_n w_z = 2 k_n delta
                    w = np.array([0.2 * along[0], 0.2 * along[1], 2.0 * spring / gr[2]])
                    offset = 0.003 * along
                else:
                    w = np.array([0.05 * along[0], 0.05 * along[1], -0.1])
                    N = spring - gr[2] * w[2]
                    limit = gr[3] * N
                    if first:                                  # T0 = -d_t w_xy: a quarter of the cone, or three times it
                        w[:2] = along * ((0.25 if branch == STICK else 3.0) * limit / gr[5])
                        offset = np.zeros(2)
                    else:                                      # T0 = -k_t offset - d_t w_xy
                        offset = along * ((0.25 if branch == STICK else 3.0) * limit / gr[4])
                v[b] = set_foot_velocity(models[b], q[b], v[b], i, w)
                cs[b, i] = [0.0, 0.0, 0.0] if first else [1.0, p[i, 0] - offset[0], p[i, 1] - offset[1]]
            ground[b] = gr
            want.append(wanted)
        calls.append(dict(q=q, v=v, tau=tau, cs=cs, ground=ground, want=want))
    return calls


# ---- the inputs of the step-alone GPU test ----
TOUCH_DOWN, LIFT_OFF = (0, 0), (1, 1)          # (instance, foot): touches down / lifts off in sub-step 2 of 3 in every round of step_cases


def step_cases(cfg, models, h, batch=4, seed=78):
    """the inputs of the ground-step GPU test, per round: wb_torque_plant_kit.step_cases' (k, q, v, control, status, pushes: a clamped joint, zero
    control actions, pushes at both ends of the tick and inside it) with cs and ground added.  The ground of instance b sits near its feet: foot
    TOUCH_DOWN starts 0.3 mm above it moving down at 1 m/s, foot LIFT_OFF 0.3 mm inside it moving up at 1 m/s, so that with S = 3 the first
    touches down and the second lifts off in sub-step 2 (asserted on the restatement by the host test); instance 3 has no ground under its lowest
    foot by 2 mm at the start of the tick and instance 2 stands 4 mm deep on its lowest foot"""
    rng = np.random.default_rng(seed)
    out = []
    for c in fd.step_cases(cfg, h, batch):
        q, v = c['q'].copy(), c['v'].copy()
        cs, ground = np.zeros((batch, 4, 3)), np.zeros((batch, 8))
        for b in range(batch):
            p = ik.forward_kinematics(models[b].legs, q[b])
            low = int(np.argmin(p[:, 2]))
            if b == TOUCH_DOWN[0]:
                z0 = p[TOUCH_DOWN[1], 2] - 3e-4
                v[b] = set_foot_velocity(models[b], q[b], v[b], TOUCH_DOWN[1], [0.1, -0.05, -1.0])
            elif b == LIFT_OFF[0]:
                z0 = p[LIFT_OFF[1], 2] + 3e-4
                v[b] = set_foot_velocity(models[b], q[b], v[b], LIFT_OFF[1], [-0.05, 0.1, 1.0])
            else:
                z0 = p[low, 2] + (4e-3 if b == 2 else -2e-3)
            ground[b] = ground_params(z0, k_n=3000.0 + 500.0 * b, d_n=40.0 + 10.0 * b, mu=0.5 + 0.1 * b, k_t=2500.0 + 300.0 * b, d_t=25.0 + 5.0 * b)
            for i in range(4):            # the feet inside the ground: every other one has been there, with an anchor 1 mm away
                if ground[b, 0] - p[i, 2] > 0 and (i + b) % 2 == 1:
                    cs[b, i] = [1.0, p[i, 0] + 1e-3 * rng.normal(), p[i, 1] + 1e-3 * rng.normal()]
        d = dict(c); d.update(q=q, v=v, cs=cs, ground=ground)
        del d['contact']
        out.append(d)
    return out


# ---- drop and settle ----
# The configuration's standing pose DROP_HEIGHT above each instance's ground, the actuators holding init_config (PD, and as feed-forward the torques
# that carry the CONTROLLER'S weight on four feet), constant control, no MPC.  Two instances: the second with a trunk heavier by SETTLE_TRUNK[1] and
# another ground height.  The values below were chosen on the restatement (test_wb_ground_plant_host.py asserts that it comes to rest under them).
SETTLE_TRUNK = (1.0, 1.2)
SETTLE_Z0 = (0.0, -0.05)
DROP_HEIGHT = 0.003
SETTLE_GROUND = dict(k_n=20000.0, d_n=400.0, mu=0.8, k_t=2000.0, d_t=100.0)
SETTLE_KP, SETTLE_KD = 100.0, 8.0
SETTLE_H, SETTLE_S, SETTLE_TICKS = 1e-3, 2, 300
V_REST = 0.2            # on |v|_inf at the end (m/s and rad/s); 0.33 at tick 50 of the restated drop
W_REST = 0.02           # on |sum F_z - m_b g| / (m_b g) at the end, m_b the plant's own mass; 0.47 at tick 50


def settle_case(cfg):
    """-> dict(models, bodies, q, v, control, kp, kd, lim, ground, weight): two instances"""
    lists = [fd.plant_cfg(cfg, f)['body_model'] for f in SETTLE_TRUNK]
    models = [kit.Model(fd.plant_cfg(cfg, bodies=bl)) for bl in lists]
    ctrl = kit.Model(cfg)
    q0 = np.array(cfg['init_config'], float)
    # the torques that carry the controller's model at rest on four feet (the smallest forces that carry the base)
    _, _, g = ctrl.robot.dynamics_terms(q0, np.zeros(18))
    Js = np.vstack([ctrl.robot.foot_jacobian_lwa(q0, i) for i in range(4)])
    F = np.linalg.lstsq(Js.T[:6], g[:6], rcond=None)[0]
    tff = (g - Js.T @ F)[6:]
    feet = ik.forward_kinematics(ctrl.legs, q0)
    n = len(models)
    q = np.tile(q0, (n, 1))
    for b in range(n):
        q[b, 2] += SETTLE_Z0[b] + DROP_HEIGHT - feet[:, 2].min()
    control = np.tile(np.concatenate([q0[7:], np.zeros(12), tff]), (n, 1))
    ground = np.array([ground_params(z, **SETTLE_GROUND) for z in SETTLE_Z0])
    return dict(models=models, bodies=lists, q=q, v=np.zeros((n, 18)), control=control, kp=np.full((n, 12), SETTLE_KP), kd=np.full((n, 12), SETTLE_KD),
                lim=np.tile(np.asarray(cfg['torque_bounds'], float), (n, 1)), ground=ground,
                weight=np.array([m.robot.mass * 9.81 for m in models]))


def settle_measures(v, sol, weight):
    """-> |v|_inf, |sum F_z - m_b g| / (m_b g) from the last sub-step's (a, F)"""
    return float(np.abs(v).max()), float(abs(sol[18:].reshape(4, 3)[:, 2].sum() - weight) / weight)


def settle_restated(cfg, ticks=SETTLE_TICKS):
    """the drop on the restatement -> per instance (q, v, cs, sol of the last sub-step, the smallest planned-stance fz seen)"""
    c = settle_case(cfg)
    ctrl = kit.Model(cfg)
    out = []
    for b, m in enumerate(c['models']):
        q, v, cs = c['q'][b], c['v'][b], NO_CONTACT
        for k in range(ticks):
            q, v, cs, info = ground_step(m, q, v, cs, c['control'][b], False, c['kp'][b], c['kd'][b], c['lim'][b], c['ground'][b], SETTLE_H, SETTLE_S, k,
                                         ctrl.mass, ctrl.Ir_inv)
        out.append((q, v, cs, info['sol']))
    return out
