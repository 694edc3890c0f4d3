"""What the tests of the rollout's full MPC update share (test_contact_feedback_host.py, test_gpu_contact_feedback.py,
test_gpu_gait_controller_rollout.py): the rule of MPC::AdjustForCurrentContacts restated on a knot table read back from the device, and the world of
the rollouts -- test_gpu_controller_rollout.py's batch with the torque-driven plant on a ground, begun at a later tick so that the first planned
touch-down (t = 0.3) comes within 70 ms --, its grounds and the host-driven chain with the feedback entry in it.  A plain module: no fixtures,
nothing pytest collects."""
import numpy as np

import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_torque_plant_kit as fd
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import PLANT_TORQUE_DRIVEN

B, H = kit.B, kit.TICK_DT
LO, TD = 0, 1                   # knot kinds (srbm_get_knots)
NEAR, GUARD = 7e-2, 1e-1        # the rule's two constants: a touch-down less than 70 ms away is moved, if the knot is within 100 ms
SUB = 4                         # sub-steps of the plant per tick


# ---- the rule on the host, from a knot table read back (srbm_get_knots) ----
def posxy(kn, e):
    """the lift-off / touch-down knots of foot e: (times, kinds, their indices in the table)"""
    nk = int(kn['nk'][e])
    idx = [i for i in range(nk) if kn['kinds'][e, i] <= TD]
    return kn['times'][e, idx], kn['kinds'][e, idx], idx


def classify(kn, e, t):
    """what the rule does to foot e at time t if it is measured in contact: 'held' (the plan has it in contact), 'moved', 'far' (70 ms or more to
    the next touch-down) or 'error'; with the time to the next touch-down.  t inside the table (no clamping)"""
    times, kinds, _ = posxy(kn, e)
    assert times[0] <= t < times[-1], (e, t, times)
    lo = max(i for i in range(len(times)) if t >= times[i])
    up = min(i for i in range(len(times)) if t < times[i])
    if kinds[lo] == TD and kinds[up] == LO:
        return 'held', None
    up_td = up
    if kinds[up] != TD:
        t2 = times[up] + 0.001
        up_td = min(i for i in range(len(times)) if t2 < times[i])
    away = abs(times[up_td] - t)
    if not away < NEAR:
        return 'far', away
    if kinds[up] != TD or abs(times[up] - t) > GUARD:
        return 'error', away
    return 'moved', away


def knot_times(g, b):
    kn = g.knots(b)
    return [kn['times'][e, :kn['nk'][e]].copy() for e in range(4)]


def traj_bytes(g):
    return np.frombuffer(bytes(g.get_trajectory()), np.uint8)


# ---- the world of 2..4: the torque-driven plant on a ground, from tick K0 on ----
class GroundWorld:
    def __init__(self, w):
        self.w = w
        self.act = (np.full((B, 12), fd.KP), np.full((B, 12), fd.KD), np.tile(np.asarray(w.cfg['torque_bounds'], float), (B, 1)))

    def start(self, k):
        """the plant's (q, v) at tick k: the targets of t = k H on the cold-started trajectories with the kit's seeded tracking error -> q, v, q_des"""
        qd, vd, _, st = self.w.base.clone().get_targets_from_traj(k * H, self.w.q0)
        assert np.all(st == 0)
        q, v = kit.first_measured(qd, vd)
        return q, v, qd

    def feet(self, q):
        return np.array([kit.ik.forward_kinematics(self.w.model.legs, q[b]) for b in range(B)])

    def plan(self, t):
        return np.array([[int(c) for c in tr.get_contacts(t)] for tr in self.w.base.get_trajectory()])

    def fresh(self, k, ground, feedback=None, kind=PLANT_TORQUE_DRIVEN, **kw):
        q, v, qd = self.start(k)
        g, R = self.w.fresh(q=q, v=v, push=False, **kw)
        R.reset(qd)
        R.set_plant(kind, *self.act, SUB)
        if ground is not None:
            R.set_ground(ground)
        if feedback is not None:
            R.set_contact_feedback(feedback)
        return g, R


def flat_ground(gw, k):
    """per instance a plane 5 mm above the lowest foot of the plant's configuration at tick k (test_gpu_wb_ground_plant.py's values)"""
    low = gw.feet(gw.start(k)[0])[:, :, 2].min(axis=1)
    return np.array([gk.ground_params(low[b] + 0.005, k_n=5000.0, d_n=60.0, mu=0.7, k_t=3000.0, d_t=40.0) for b in range(B)])


def raised_ground(gw, k):
    """instances 0 and 2 as flat_ground; 1 and 3 raised so that their swing feet land early: 4 mm above the swing feet of tick k (1), 12 mm below
    them (3: they touch a little later).  The stance feet of a raised instance then stand that deep in the ground: its normal stiffness is the one
    at which two feet that deep carry the robot, k_n = m g / (2 depth), so that the ground neither throws it up nor lets it fall"""
    q = gw.start(k)[0]
    feet, plan = gw.feet(q), gw.plan(k * H)
    ground = flat_ground(gw, k)
    for b, dz in ((1, 0.004), (3, -0.012)):
        swing = [e for e in range(4) if not plan[b, e]]
        assert len(swing) == 2
        z0 = feet[b, swing, 2].min() + dz
        depth = z0 - feet[b, :, 2].min()
        assert depth > 0.01, (b, depth)
        ground[b] = gk.ground_params(z0, k_n=gw.w.cfg['mass'] * 9.81 / (2 * depth), d_n=60.0, mu=0.7, k_t=3000.0, d_t=40.0)
    return ground


def feedback_chain(Dev, g, R, q, v, cs, first, ticks, tpu, feedback=True, update=None, ground=True):
    """the loop driven from the host: srbm_control_tick_dev, at an update tick srbm_controller_contact_feedback_dev (feedback), the plant step
    (srbm_wb_ground_step_dev, or srbm_wb_plant_step_dev with ground=False), at an update tick srbm_get_real_time_update_dev -- or update(k, state,
    time, ee) on what the tick wrote, read back to the host.  Ends with the batch's own plant and contact state set to what the chain left;
    -> the feedback record the chain counted (set_state resets it)"""
    T = ControlTick(g)
    n = g.batch
    d = dict(q=Dev(q), v=Dev(v), cs=Dev(cs), t=Dev(np.zeros(n)), control=Dev(np.zeros((n, 36))), qp_sol=Dev(np.zeros((n, 30))),
             status=Dev(np.zeros((n, 2), np.int32)), contact=Dev(np.zeros((n, 4), np.int32)), state=Dev(np.zeros((n, 13))), ee=Dev(np.zeros((n, 4, 3))))
    for k in range(first, first + ticks):
        g.synchronize()
        d['t'].put(np.full(n, k * H))
        is_update = k > 0 and k % tpu == 0
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        if is_update and feedback:
            R.contact_feedback_dev(d['t'].p.value, d['cs'].p.value)
        if ground:
            R.ground_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['control'].p.value, d['status'].p.value)
        else:
            R.plant_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['qp_sol'].p.value, d['status'].p.value)
        if is_update and update is None:
            g.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
        elif is_update:
            g.synchronize()
            update(k, d['state'].get(), d['t'].get(), d['ee'].get())
    g.synchronize()
    fb = R.contact_feedback()
    R.set_state(d['q'].get(), d['v'].get())
    R.set_contact_state(d['cs'].get())
    return fb


def ground_snapshot(snapshot, w, g, R, next_tick):
    s = snapshot(w, g, R, next_tick)
    s['cs'] = R.contact_state()
    return s
