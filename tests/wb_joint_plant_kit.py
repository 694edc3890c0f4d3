"""What the tests of the torque-driven plant's joint model (test_wb_joint_plant_host.py, test_gpu_wb_joint_plant.py) share, built on the restatements
of wb_torque_plant_kit.py, wb_ground_plant_kit.py and wb_terrain_plant_kit.py: the law of include/srbm_rti.h ("a joint model") as a Python loop on
floats, statement by statement; the armature as a wrapper of the plant's model whose M carries it, so that the three restated solves take it
unchanged; the step on the three surfaces with the law between the command and the solve; the seeded inputs of the tests with their branch
margins; the A1 fixture; and the limp drop with its recorded constants.  A plain module: no fixtures, nothing pytest collects."""
import json
import os

import numpy as np

import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_terrain_plant_kit as tk
import wb_torque_plant_kit as fd
from controller_rollout_kit import ik

INF = float('inf')
JB, JIA, JFC, JVS, JQMIN, JQMAX, JT = range(7)
HELD, GROUND, TERRAIN = 'held', 'ground', 'terrain'
FIXTURE = os.path.join(kit.ROOT, 'tests', 'golden', 'a1_joint_model.json')


def joint(b=0.0, ia=0.0, fc=0.0, vs=0.0, q_min=-INF, q_max=INF, T=0.0):
    return np.array([b, ia, fc, vs, q_min, q_max, T, 0.0])


def transparent(batch=None):
    """b = I_a = f_c = v_s = T = 0 and infinite ranges -> [12][8], or [batch][12][8]"""
    J = np.tile(joint(), (12, 1))
    return J if batch is None else np.tile(J, (batch, 1, 1))


def alpha(T, hs):
    if T == 0.0:
        return 0.0
    s = T + hs
    return hs / s


def joint_law(c, al, kl, dl, cmd, q, v, tau_m):
    """the law for one joint and one sub-step, on Python floats (IEEE doubles, one rounded operation per statement) -> t, tau_m, dict(exc, fr, lag,
    branch: what was taken, margins: the distances of the inputs to the branch boundaries that exist for this joint)"""
    c = [float(x) for x in c]
    kl, dl, cmd, q, v, tau_m = float(kl), float(dl), float(cmd), float(q), float(v), float(tau_m)
    branch, margins = [], []
    if c[JT] == 0.0:
        tau_m = cmd
    else:
        d = cmd - tau_m
        ad = al * d
        tau_m = tau_m + ad
        branch.append('lag')
    lag = abs(cmd - tau_m)
    t = tau_m
    pd = pc = 0.0
    if c[JB] != 0.0:
        pd = c[JB] * v
        t = t - pd
        branch.append('damped')
    if c[JFC] != 0.0:
        r = v / c[JVS]
        margins.append(abs(abs(r) - 1.0))
        branch.append('band' if abs(r) < 1.0 else ('sat+' if r > 0 else 'sat-'))
        r = min(max(r, -1.0), 1.0)
        pc = c[JFC] * r
        t = t - pc
    fr = abs(pd + pc)
    exc = 0.0
    e = c[JQMIN] - q
    if np.isfinite(e):
        margins.append(abs(e))
    if e > 0.0:
        sl = kl * e
        dd = dl * v
        sl = sl - dd
        margins.append(abs(sl))
        branch.append('lower' if sl > 0.0 else 'lower-clamped')
        sl = max(sl, 0.0)
        t = t + sl
        exc = e
    e = q - c[JQMAX]
    if np.isfinite(e):
        margins.append(abs(e))
    if e > 0.0:
        su = kl * e
        du = dl * v
        su = su + du
        margins.append(abs(su))
        branch.append('upper' if su > 0.0 else 'upper-clamped')
        su = max(su, 0.0)
        t = t - su
        exc = e
    return t, tau_m, dict(exc=exc, fr=fr, lag=lag, branch=branch, margins=margins)


def record_fold(rec, n, over, exc, fr, lag, mask):
    rec = np.array(rec, float)
    rec[0] += n; rec[1] += over
    rec[2] = max(rec[2], exc); rec[3] = max(rec[3], fr); rec[4] = max(rec[4], lag)
    rec[5] = float(int(rec[5]) | mask)
    return rec


def law_substep(J, stops, hs, cmd, q_j, v_j, js):
    """the 12 joints of one instance in one sub-step -> t[12], js[12], the infos"""
    t, out, infos = np.zeros(12), np.zeros(12), []
    for j in range(12):
        t[j], out[j], info = joint_law(J[j], alpha(float(J[j][JT]), hs), stops[0], stops[1], cmd[j], q_j[j], v_j[j], js[j])
        infos.append(info)
    return t, out, infos


def fold_infos(history):
    """the infos of the sub-steps of a launch -> (n, over, exc, fr, lag, mask) for record_fold"""
    over = mask = 0
    exc = fr = lag = 0.0
    for infos in history:
        m = sum(1 << j for j, i in enumerate(infos) if i['exc'] > 0.0)
        over += m != 0
        mask |= m
        exc = max([exc] + [i['exc'] for i in infos]); fr = max([fr] + [i['fr'] for i in infos]); lag = max([lag] + [i['lag'] for i in infos])
    return len(history), over, exc, fr, lag, mask


# ---- the armature: a model whose M carries it ----
class _ArmatureRobot:
    def __init__(self, robot, ia):
        self._robot, self._ia = robot, np.asarray(ia, float)

    def __getattr__(self, name):
        return getattr(self._robot, name)

    def dynamics_terms(self, q, v):
        M, Cv, g = self._robot.dynamics_terms(q, v)
        M = np.array(M, float)
        for j in range(12):
            if self._ia[j] != 0.0:
                M[6 + j, 6 + j] = M[6 + j, 6 + j] + self._ia[j]
        return M, Cv, g


class WithArmature:
    """model (controller_rollout_kit.Model of the plant's bodies) with I_a[12] on the joints' diagonal entries of M"""

    def __init__(self, model, ia):
        self._model = model
        self.robot = _ArmatureRobot(model.robot, ia)

    def __getattr__(self, name):
        return getattr(self._model, name)


def dynamics(surface, model, J, q, v, tau, contact=None, cs=None, gr=None, terrain=None):
    """(a, F) with tau the net joint torque and the armatures of J on M -> sol[30], cs_out (None with the feet held), infos"""
    m = WithArmature(model, np.asarray(J, float)[:, JIA])
    if surface == HELD:
        return fd.forward_dynamics(m.robot, q, v, tau, contact), None, None
    if surface == GROUND:
        return gk.ground_dynamics(m, q, v, tau, cs, gr)
    return tk.terrain_dynamics(m, q, v, tau, cs, gr, terrain)


def residual_with_armature(model, J, q, v, sol, tau, F, contact):
    """the dynamics residual of controller_rollout_kit with I_a a on the joint rows"""
    res = kit.dynamics_residual(model, q, v, sol[:18], tau, F, contact)
    res = np.array(res, float)
    res[6:] += np.asarray(J, float)[:, JIA] * sol[6:18]
    return res


def joint_step(surface, model, q, v, control, off, kp, kd, lim, J, stops, js, h, S, k, mass, Ir_inv, push=None, contact=None, cs=None, gr=None, terrain=None):
    """tick k of the torque-driven plant with a joint model for one instance: S sub-steps of h / S -> q+, v+, cs+ (None with the feet held), js+,
    dict(pushed, clamped, deviation, sol, tau of the last sub-step, history: the law's infos of every sub-step, contact_history: the ground's)"""
    q, v, js = np.array(q, float), np.array(v, float), np.array(js, float)
    cs = None if cs is None else np.array(cs, float).reshape(4, 3)
    J = np.asarray(J, float)
    hs = h / S
    pushed = push is not None and kit.push_applies(k * h, h, push[0])
    history, contact_history = [], []
    for s in range(S):
        cmd, clamped, _ = fd.torque_law(control, q, v, kp, kd, lim, off)
        tau, js, infos = law_substep(J, stops, hs, cmd, q[7:], v[6:], js)
        history.append(infos)
        dev = float(np.abs(tau - np.asarray(control, float)[24:]).max())
        sol, cs_new, cinfos = dynamics(surface, model, J, q, v, tau, contact, cs, gr, terrain)
        if surface != HELD:
            cs = cs_new
            contact_history.append(cinfos)
        hv = hs * sol[:18]
        v = v + hv
        if s == S - 1 and pushed:
            imp = np.asarray(push[1], float)
            v[:3] = v[:3] + imp[:3] / mass
            v[3:6] = v[3:6] + Ir_inv @ imp[3:]
        q = ik.integrate(q, v, hs)
    return q, v, cs, js, dict(pushed=pushed, clamped=clamped, deviation=dev, sol=sol, tau=tau, history=history, contact_history=contact_history)


# ---- the A1 fixture ----
def load_fixture():
    return json.load(open(FIXTURE))


A1_STICTION_BAND = 0.1          # rad/s; the fixture's simulator treats dry friction as a constraint and has no band
A1_MOTOR_T = 2e-3               # s; the fixture has no motor lag
A1_STOPS = (200.0, 2.0)         # k_l, d_l: with I_link + I_a >= 0.01 kg m^2 the stop's rate sqrt(k_l / I) <= 141 rad/s, resolved by hs <= 1 / 3 ms


# ---- the branch table of the law ----
# per joint of instance 0 of law_cases: the branch set that joint_law must report in every sub-step
BRANCH_TABLE = [['damped'], ['lag', 'damped', 'lower'], ['lower-clamped'], ['damped', 'upper'], ['lag', 'upper-clamped'], ['band'], ['lag', 'sat+'],
                ['damped', 'sat-'], ['damped', 'band'], ['lag'], [], ['lag', 'damped', 'sat-', 'lower']]
LAW_S, LAW_H = 3, 1e-2
MARGIN = 1e-6


def law_cases(seed=31):
    """-> dict(joints[3][12][8], stops[3][2], cmd, q_j, v_j [LAW_S][3][12], off[3], js[3][12], want): instance 0 has its 12 joints in the branches of
    BRANCH_TABLE (inside the range; below q_min approaching, and receding so fast that the fmax clamps; above q_max likewise; friction inside the
    band and saturated in both signs; T = 0 and T > 0; every coefficient zero), instance 1 is the transparent model, instance 2 is instance 0 with
    its actuators off.  The states drift a little from sub-step to sub-step and stay in their branches"""
    rng = np.random.default_rng(seed)
    kl, dl = 150.0, 3.0
    q = rng.uniform(-0.5, 0.5, 12)
    v = rng.uniform(-0.4, 0.4, 12)
    J = np.zeros((12, 8))
    J[0] = joint(b=1.5, q_min=q[0] - 0.3, q_max=q[0] + 0.4)
    v[1] = -0.3; J[1] = joint(b=0.7, q_min=q[1] + 0.02, q_max=q[1] + 1.0, T=4e-3)                       # below, approaching: k e - d v > 0
    v[2] = 4.0; J[2] = joint(q_min=q[2] + 0.03, q_max=q[2] + 2.0)                                       # below, receding: 150 * 0.03 - 3 * 4 < 0
    v[3] = 0.25; J[3] = joint(b=2.0, q_min=q[3] - 1.0, q_max=q[3] - 0.05)                               # above, approaching
    v[4] = -5.0; J[4] = joint(q_min=q[4] - 2.0, q_max=q[4] - 0.04, T=1e-2)                              # above, receding: 150 * 0.04 - 3 * 5 < 0
    v[5] = 0.02; J[5] = joint(fc=0.2, vs=0.1)
    v[6] = 0.35; J[6] = joint(fc=0.3, vs=0.1, T=2e-3)
    v[7] = -0.5; J[7] = joint(b=1.0, fc=0.2, vs=0.05)
    v[8] = -0.03; J[8] = joint(b=1.0, ia=0.01, fc=0.2, vs=0.1, q_min=q[8] - 0.5, q_max=q[8] + 0.5)      # T = 0 with everything else
    J[9] = joint(T=5e-3, q_min=q[9] - 0.5)
    J[10] = joint(q_min=q[10] - 0.2, q_max=q[10] + 0.2)                                                 # every coefficient zero, finite range, inside
    v[11] = -0.6; J[11] = joint(b=1.0, ia=0.02, fc=0.25, vs=0.1, q_min=q[11] + 0.05, q_max=q[11] + 3.0, T=3e-3)
    joints = np.stack([J, transparent(), J])
    stops = np.array([[kl, dl], [kl, dl], [kl, dl]])
    drift = np.arange(LAW_S)[:, None, None]
    q_j = np.tile(q, (LAW_S, 3, 1)) + 1e-3 * drift * rng.uniform(-1, 1, (1, 3, 12))
    v_j = np.tile(v, (LAW_S, 3, 1)) + 1e-3 * drift * rng.uniform(-1, 1, (1, 3, 12))
    cmd = rng.uniform(-20, 20, (LAW_S, 3, 12))
    js = rng.uniform(-5, 5, (3, 12))
    return dict(joints=joints, stops=stops, cmd=cmd, q_j=q_j, v_j=v_j, off=np.array([0, 0, 1], np.int32), js=js,
                want=[BRANCH_TABLE, [[]] * 12, BRANCH_TABLE])


def law_restated(c):
    """law_cases' dict -> tau[LAW_S][3][12], js[3][12], jrec[3][8], the smallest margin, the branches seen [instance][sub-step][joint]"""
    S, B = c['cmd'].shape[:2]
    hs = LAW_H / S
    tau, js, jrec = np.zeros((S, B, 12)), c['js'].copy(), np.zeros((B, 8))
    margin, seen = INF, []
    for b in range(B):
        history = []
        for s in range(S):
            cmd = np.zeros(12) if c['off'][b] else c['cmd'][s, b]
            tau[s, b], js[b], infos = law_substep(c['joints'][b], c['stops'][b], hs, cmd, c['q_j'][s, b], c['v_j'][s, b], js[b])
            history.append(infos)
            margin = min([margin] + [m for i in infos for m in i['margins']])
        jrec[b] = record_fold(jrec[b], *fold_infos(history))
        seen.append([[i['branch'] for i in infos] for infos in history])
    return tau, js, jrec, margin, seen


# ---- the inputs of the GPU tests ----
def solve_armatures(batch=4, seed=41):
    """I_a from 0 to 0.1 mixed within an instance (some exactly 0: those entries of M are not touched) -> joints[batch][12][8], otherwise transparent"""
    rng = np.random.default_rng(seed)
    J = transparent(batch)
    ia = rng.uniform(0.0, 0.1, (batch, 12))
    ia[:, ::4] = 0.0
    ia[1, 5] = 0.1
    J[:, :, JIA] = ia
    return J


CROSSING = (2, 7)               # (instance, joint) of step_joints: crosses its upper stop in sub-step 2 of 3
TABLE = 3                       # the instance of step_joints that carries BRANCH_TABLE's kinds of joints (it has no torque limit and no foot velocity set)
STEP_RATES = {1: -0.3, 2: 4.0, 3: 0.25, 4: -5.0, 5: 0.02, 6: 0.35, 7: -0.5, 8: -0.03, 11: -0.6}         # joint -> its rate on instance TABLE, as in law_cases


def step_rates(cases):
    """the rounds of a step_cases of the three plant kits with the joint rates the branches need: STEP_RATES on instance TABLE, 2 rad/s on the joint
    that crosses its stop (in place, on copies of v)"""
    for c in cases:
        c['v'] = c['v'].copy()
        for j, r in STEP_RATES.items():
            c['v'][TABLE, 6 + j] = r
        c['v'][CROSSING[0], 6 + CROSSING[1]] = 2.0
    return cases


def step_joints(cases, batch=4):
    """the joint models of the step test on step_rates(...) of a kit's step cases: per round joints[batch][12][8] and stops[batch][2].  Instance
    TABLE carries BRANCH_TABLE's kinds of joints placed around its own q of the round, instance 1 A1-like values on every joint, instance 2 has joint
    CROSSING[1] 1 mrad under its upper stop moving up at 2 rad/s, so that with S = 3 and ticks of 10 ms it crosses in sub-step 2, instance 0
    armature and lag alone"""
    out = []
    for c in cases:
        q = c['q']
        J = transparent(batch)
        stops = np.array([[80.0, 0.5], [200.0, 2.0], [120.0, 1.0], [150.0, 3.0]])
        qa = q[TABLE, 7:]
        T = J[TABLE]
        T[0] = joint(b=1.5, ia=0.01, q_min=qa[0] - 0.3, q_max=qa[0] + 0.4)
        T[1] = joint(b=0.7, q_min=qa[1] + 0.02, q_max=qa[1] + 1.0, T=4e-3)
        T[2] = joint(q_min=qa[2] + 0.03, q_max=qa[2] + 2.0, ia=0.03)
        T[3] = joint(b=2.0, q_min=qa[3] - 1.0, q_max=qa[3] - 0.05)
        T[4] = joint(q_min=qa[4] - 2.0, q_max=qa[4] - 0.04, T=1e-2)
        T[5] = joint(fc=0.2, vs=0.1)
        T[6] = joint(fc=0.3, vs=0.1, T=2e-3)
        T[7] = joint(b=1.0, fc=0.2, vs=0.05)
        T[8] = joint(b=1.0, ia=0.01, fc=0.2, vs=0.1, q_min=qa[8] - 0.5, q_max=qa[8] + 0.5)
        T[9] = joint(T=5e-3, q_min=qa[9] - 0.5)
        T[10] = joint(q_min=qa[10] - 0.2, q_max=qa[10] + 0.2)
        T[11] = joint(b=1.0, ia=0.02, fc=0.25, vs=0.1, q_min=qa[11] + 0.05, q_max=qa[11] + 3.0, T=3e-3)
        J[1] = np.tile(joint(b=1.0, ia=0.01, fc=0.2, vs=A1_STICTION_BAND, q_min=-3.0, q_max=4.5, T=A1_MOTOR_T), (12, 1))
        J[2, CROSSING[1]] = joint(b=0.5, ia=0.02, q_min=-INF, q_max=q[2, 7 + CROSSING[1]] + 1e-3)
        J[0] = np.tile(joint(ia=0.015, T=3e-3), (12, 1))
        out.append((J, stops))
    return out


# ---- the limp drop ----
# A crouched pose (DROP_POSE on every leg: the calves DROP_POSE[2] - q_min = 6.5 mrad inside their lower stops) DROP_HEIGHT above the ground, a zero
# control action (the actuators off: only the joints' own damping, friction and stops act), one instance, the A1 fixture's joint values with
# A1_STICTION_BAND and A1_STOPS.  The feet touch down after 8 ms, the weight folds the calves into their stops after about 25 ms, and the stops
# carry it from there.  300 ticks of the restatement take half a minute on a CPU, so the drop is DROP_TICKS long; the check is the issue's.  The
# constants were measured on the restatement (test_wb_joint_plant_host.py runs it and holds them to 5 %).
DROP_H, DROP_S, DROP_TICKS = 1e-3, 4, 60
DROP_HEIGHT = 0.0003
DROP_POSE = (0.0, 1.25, -2.69)
DROP_GROUND = dict(k_n=20000.0, d_n=400.0, mu=0.8, k_t=2000.0, d_t=100.0)
DROP_CHECK_TICKS = 10           # the ticks over which device and restatement are compared to the step tests' bound
DROP_EXCURSION = 0.0324         # rad: the largest excursion beyond a range over the drop (the four calves, mask 2340); measured 0.0324
DROP_V_END = 0.875              # |v|_inf at the end (rad/s: the joints still fold into their stops); measured 0.8753


def drop_case(cfg):
    from srbm_loader import joints as jm
    model = kit.Model(cfg)
    J, lim = jm.a1_model(load_fixture(), A1_STICTION_BAND)
    q = np.array(cfg['init_config'], float)
    q[7:] = np.tile(DROP_POSE, 4)
    feet = ik.forward_kinematics(model.legs, q)
    q[2] += DROP_HEIGHT - feet[:, 2].min()
    return dict(model=model, joints=J, stops=np.array(A1_STOPS), lim=lim, q=q, v=np.zeros(18), control=np.zeros(36), ground=gk.ground_params(0.0, **DROP_GROUND))


def drop_restated(cfg, ticks=DROP_TICKS, keep=DROP_CHECK_TICKS):
    """-> dict(q, v, cs, js, jrec after `ticks`, first: the (q, v, cs, js) after each of the first `keep` ticks)"""
    c = drop_case(cfg)
    q, v, cs, js, jrec = c['q'], c['v'], gk.NO_CONTACT, np.zeros(12), np.zeros(8)
    first = []
    for k in range(ticks):
        q, v, cs, js, info = joint_step(GROUND, c['model'], q, v, c['control'], True, np.zeros(12), np.zeros(12), c['lim'], c['joints'], c['stops'], js, DROP_H,
                                        DROP_S, k, c['model'].mass, c['model'].Ir_inv, cs=cs, gr=c['ground'])
        jrec = record_fold(jrec, *fold_infos(info['history']))
        if k < keep:
            first.append((q, v, cs, js))
    return dict(q=q, v=v, cs=cs, js=js, jrec=jrec, first=first)
