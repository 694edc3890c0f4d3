"""What the control-tick tests (test_gpu_control_tick.py, test_control_tick_host.py) share: numpy restatements of MPCController::ReconstructState
(controllers/mpc_controller.cpp:229-271) and of the stacking of force_target_ (:181-188, as bench.py's wbc segment writes it), and the chain of
the single entries the one-call tick (srbm_control_tick) is held to.  A plain module: no fixtures, nothing pytest collects."""
import numpy as np

TICK_KEYS = ('control', 'qp_sol', 'targets_status', 'qp_status', 'qp_iters', 'q_des', 'v_des', 'contact')       # bitwise: tick == chain


def reconstruct_state(q, v, mass, Ir):
    """ReconstructState: [p, m v_lin, firstOrderNormalize(quaternion xyzw), Ir w] (the vel_frame lines of :251-255 have no effect).
    q [..., 19], v [..., 18] -> [..., 13]"""
    q, v, Ir = np.asarray(q, float), np.asarray(v, float), np.asarray(Ir, float).reshape(3, 3)
    s = np.zeros(q.shape[:-1] + (13,))
    s[..., 0:3] = q[..., 0:3]
    s[..., 3:6] = v[..., 0:3] * mass
    x, y, z, w = (q[..., 3 + i] for i in range(4))
    a = (3.0 - (x * x + y * y + z * z + w * w)) / 2.0                      # pinocchio::quaternion::firstOrderNormalize
    s[..., 6:10] = q[..., 3:7] * a[..., None]
    for i in range(3):
        s[..., 10 + i] = Ir[i, 0] * v[..., 3] + Ir[i, 1] * v[..., 4] + Ir[i, 2] * v[..., 5]
    return s


def stack_forces(f_des, con):
    """force_target_: 3 per foot in contact, stacked in foot order (stable sort of the feet by "not in contact"), zero behind them.
    f_des [B, 4, 3], con [B, 4] -> [B, 12]"""
    f_des, con = np.asarray(f_des, float), np.asarray(con)
    order = np.argsort(con == 0, axis=1, kind='stable')
    return (np.take_along_axis(f_des, order[:, :, None], axis=1) * (np.take_along_axis(con, order, axis=1) > 0)[:, :, None]).reshape(len(con), 12)


def measured(q_des, v_des, rng, scale=0.01):
    """the "measured" state of a tick: the targets with a tracking error on the joints and on every velocity"""
    q = q_des.copy(); q[:, 7:] += rng.normal(size=(len(q), 12)) * scale
    return q, v_des + rng.normal(size=v_des.shape) * scale


def chain_targets(g, time, q_guess):
    """the first half of the chain: GetTargetsFromTraj, GetDesiredContacts, the stacked force targets"""
    q_des, v_des, f_des, st = g.get_targets_from_traj(time, q_guess)
    _, _, con = g.eval_trajectory(time)
    return dict(q_des=q_des, v_des=v_des, targets_status=st, contact=con, force_target=stack_forces(f_des, con))


def chain_qp(g, tg, q, v):
    """... and the second: QPControl::ComputeControlAction on the measured (q, v); the dict a tick is compared with (TICK_KEYS)"""
    ctl, sol, st, it = g.qp_control(q, v, tg['contact'], tg['q_des'], tg['v_des'], tg['force_target'])
    return dict(tg, control=ctl, qp_sol=sol, qp_status=st, qp_iters=it)


def assert_tick_equals_chain(out, ref, where, rows=None):
    rows = slice(None) if rows is None else rows
    for k in TICK_KEYS:
        a, b = np.asarray(out[k])[rows], np.asarray(ref[k])[rows]
        assert a.shape == b.shape and a.dtype.kind == b.dtype.kind, (where, k, a.shape, b.shape)
        if a.tobytes() != b.astype(a.dtype).tobytes():
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError('%s: %s differs from the chain at rows %s' % (where, k, bad[:8].tolist()))
