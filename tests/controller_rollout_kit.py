"""What the whole-controller rollout tests (test_controller_rollout_host.py, test_gpu_controller_rollout.py) share: a numpy restatement of the loop
of srbm_controller_advance -- control tick, whole-body plant step, MPC update -- built from control_tick_kit.reconstruct_state,
ik_numpy.targets_from_traj / forward_kinematics / integrate and the whole-body QP of wbc_numpy, on trajectory records (host.Trajectory) that the
caller reads back from the device (GPU tests) or takes from the CPU oracle (host tests).  A plain module: no fixtures, nothing pytest collects."""
import os
import sys

import numpy as np

from control_tick_kit import reconstruct_state, stack_forces
from oracle_py import qp_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ik_numpy as ik
import wbc_numpy as wbc

# the shapes of every GPU test: 4 Config-B instances, ticks of 10 ms (35 of them cross the first contact switch at 0.3 s), an MPC update every 5,
# instance PUSHED pushed in tick PUSH_TICK
B, TICK_DT, TPU, NTICKS = 4, 0.01, 5, 35
PUSHED, PUSH_TICK = 2, 3
PUSH_TIME = 3.5 * TICK_DT
IMPULSE = np.array([1.5, -1.0, 0.5, 0.05, -0.08, 0.04])
NOISE_SEED = 21         # of the tracking error on the first measured (q, v); chosen in test_controller_rollout_host.py


def push_applies(t_k, h, push_time):
    """the push rule of the plant step: t_k < push_time <= t_k + h, with t_k + h one rounded sum"""
    tn = t_k + h
    return bool(push_time > t_k and push_time <= tn)


def plant_step(q, v, a, h, k, mass, Ir_inv, coast=False, push=None):
    """one instance: (q+, v+, pushed).  a: qp_sol (its first 18 entries are used); push: (time, impulse[6]) or None"""
    acc = np.zeros(18) if coast else np.asarray(a, float)[:18]
    hv = h * acc
    vp = np.asarray(v, float) + hv
    pushed = push is not None and push_applies(k * h, h, push[0])
    if pushed:
        imp = np.asarray(push[1], float)
        vp[:3] = vp[:3] + imp[:3] / mass
        vp[3:6] = vp[3:6] + Ir_inv @ imp[3:]
    return ik.integrate(np.asarray(q, float), vp, h), vp, pushed


class Model:
    def __init__(self, cfg):
        self.cfg = cfg
        self.legs = np.array(cfg['leg_origins'], float)
        self.robot = wbc.Robot(cfg)
        self.mass, self.Ir = cfg['mass'], np.array(cfg['Ir'], float)
        self.Ir_inv = np.linalg.inv(self.Ir)


def unstack_forces(x, contact):
    """qp_sol -> F[4][3]: the forces behind the 18 accelerations, 3 per foot in contact in foot order; zero for a foot not in contact"""
    F, j = np.zeros((4, 3)), 0
    for i in range(4):
        if contact[i]:
            F[i] = x[18 + 3 * j:21 + 3 * j]; j += 1
    return F


def restated_tick(model, traj, t, q, v, q_des):
    """MPCController::ComputeControlAction for one instance on the trajectory record `traj`: dict(q_des, v_des, contact, control[36], qp_sol[30],
    targets_ok, qp_status, coast, state[13], ee[4][3])"""
    qd, vd, fd, ok = ik.targets_from_traj(model.legs, traj.get_states(), traj.init_time, traj.node_dt, model.mass, model.Ir_inv,
                                          lambda e, tt: traj.get_end_effector_location(e, tt), lambda e, tt: traj.get_force(e, tt), t, q_des)
    con = np.array([int(c) for c in traj.get_contacts(t)])
    nc = int(con.sum())
    ft = stack_forces(fd[None], con[None])[0]
    ctl, x, st = wbc.control_action(model.robot, model.cfg, q, v, con, qd, vd, ft[:3 * nc], qp_solve)
    coast = st > 1
    sol = np.zeros(30)
    if coast:
        ctl = np.zeros(36)
    else:
        sol[:18 + 3 * nc] = x
    return dict(q_des=qd, v_des=vd, contact=con, control=ctl, qp_sol=sol, targets_ok=ok, qp_status=st, coast=coast,
                state=reconstruct_state(q, v, model.mass, model.Ir), ee=ik.forward_kinematics(model.legs, q))


def dynamics_residual(model, q, v, a, tau, F, contact):
    """the 18 rows of M a + C v + g - S' tau - Js' F through wbc_numpy's RNEA and foot Jacobians.  F[4][3] per foot (only feet in contact count)"""
    res = model.robot.rnea(q, v, a)
    res[6:] -= tau
    for i in range(4):
        if contact[i]:
            res -= model.robot.foot_jacobian_lwa(q, i).T @ np.asarray(F, float).reshape(4, 3)[i]
    return res


class RestatedLoop:
    """the loop of srbm_controller_advance for a list of instances.  trajs: one trajectory record per instance; solve(b, state13, t, ee) -> the new
    record of instance b (the MPC update; None: the loop never updates)"""

    def __init__(self, model, trajs, q, v, q_des, push_time=None, impulse=None, solve=None):
        self.model, self.trajs, self.solve = model, list(trajs), solve
        self.q, self.v, self.q_des = np.array(q, float), np.array(v, float), np.array(q_des, float)
        self.push_time, self.impulse = push_time, impulse

    def tick(self, k, h, ticks_per_update):
        """-> one dict per instance: restated_tick's, with pushed, update, q+, v+"""
        out = []
        update = k > 0 and k % ticks_per_update == 0
        for b in range(len(self.q)):
            r = restated_tick(self.model, self.trajs[b], k * h, self.q[b], self.v[b], self.q_des[b])
            push = None if self.push_time is None else (self.push_time[b], self.impulse[b])
            qn, vn, pushed = plant_step(self.q[b], self.v[b], r['qp_sol'], h, k, self.model.mass, self.model.Ir_inv, r['coast'], push)
            r.update(pushed=pushed, update=update, q_next=qn, v_next=vn)
            if update and self.solve is not None:
                self.trajs[b] = self.solve(b, r['state'], k * h, r['ee'])
            self.q[b], self.v[b], self.q_des[b] = qn, vn, r['q_des']
            out.append(r)
        return out


def first_measured(q_des, v_des, seed=NOISE_SEED, scale=0.01):
    """the plant's first (q, v): the targets of tick 0 with a seeded tracking error on the joints and on every velocity (control_tick_kit.measured)"""
    rng = np.random.default_rng(seed)
    q = np.array(q_des, float); q[:, 7:] += rng.normal(size=(len(q), 12)) * scale
    return q, np.array(v_des, float) + rng.normal(size=np.shape(v_des)) * scale


def pushes(batch=B):
    """instance PUSHED is pushed inside tick PUSH_TICK; the others have a push record that never fires"""
    t = np.full(batch, -1.0); t[PUSHED] = PUSH_TIME
    imp = np.zeros((batch, 6)); imp[PUSHED] = IMPULSE
    return t, imp
