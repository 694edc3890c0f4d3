"""The control tick as one entry (include/srbm_rti.h: srbm_control_tick[_dev], srbm_control_tick_reset):
MPCController::ComputeControlAction (controllers/mpc_controller.cpp:120-227) for every instance of a host.BatchMPC, with the controller's q_des_ held
by the batch.  A module of its own beside host.py, as gait_rollout.py: it calls through the library `host.declare` has typed."""
import ctypes as C

import numpy as np

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


class ControlTick:
    """mpc: a host.BatchMPC with leg kinematics and a whole-body model (a cfg with 'init_config' sets both)"""

    def __init__(self, mpc):
        self.mpc, self.L = mpc, mpc.L

    def reset(self, q_des):
        """control_tick_reset: MPCController's q_des_ (the IK guess of the next tick) for every instance, one q[19] or [batch][19]"""
        m = self.mpc
        m._chk(self.L.srbm_control_tick_reset(m.h, _d(m._bcast(q_des, 19))))

    def tick(self, q, v, time):
        """control_tick: ReconstructState + GetTargetsFromTraj + GetDesiredContacts + the stacking of the force targets +
        QPControl::ComputeControlAction on the measured q[batch][19], v[batch][18] at time (one value or [batch]).  Synchronous.
        -> dict(control [batch][36], qp_sol [batch][30], targets_status, qp_status, qp_iters, q_des, v_des, contact [batch][4], state [batch][13],
        ee [batch][4][3])"""
        m = self.mpc
        B = m.batch
        qq, vv, t = m._bcast(q, 19), m._bcast(v, 18), m._times(time)
        ctl, sol, st = np.zeros((B, 36)), np.zeros((B, 30)), np.zeros((B, 2), np.int32)
        qd, vd, con, x, ee = np.zeros((B, 19)), np.zeros((B, 18)), np.zeros((B, 4), np.int32), np.zeros((B, 13)), np.zeros((B, 4, 3))
        m._chk(self.L.srbm_control_tick(m.h, _d(qq), _d(vv), _d(t), _d(ctl), _d(sol), _i(st), _d(qd), _d(vd), _i(con),
                                        _d(x), _d(ee)))
        return dict(control=ctl, qp_sol=sol, targets_status=st[:, 0].copy(), qp_status=st[:, 1] & 255, qp_iters=st[:, 1] >> 8, q_des=qd, v_des=vd,
                    contact=con, state=x, ee=ee)

    def tick_dev(self, q, v, time, control, qp_sol, status, q_des=None, v_des=None, contact=None, state=None, ee=None):
        """control_tick_dev: the same on device pointers (ints; the last five may be None): asynchronous on the batch's stream, no copy,
        no synchronisation"""
        self.mpc._chk(self.L.srbm_control_tick_dev(self.mpc.h, q, v, time, control, qp_sol, status, q_des, v_des, contact, state, ee))
