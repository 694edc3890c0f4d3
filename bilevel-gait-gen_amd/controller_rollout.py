"""Whole-controller rollouts (include/srbm_rti.h: srbm_controller_advance, srbm_wb_plant_*, srbm_tick_log_*): the loop of the reference's top-level
program (test/simulation_mpc.cpp:186-215) for every instance of a host.BatchMPC -- MPCController::ComputeControlAction every tick, an MPC update
every `ticks_per_update` ticks, and between them a whole-body plant that integrates the accelerations of the whole-body QP (it has no ground, no
joint PD loop and no AdjustForCurrentContacts: the header says what that means).  A module of its own beside host.py, as control_tick.py and
mpc_period.py are: it calls through the library `host.declare` has typed, and tests/test_abi_prototypes.py keeps the method list of host.BatchMPC
as it stands.

    R = ControllerRollout(mpc)            mpc: a BatchMPC with leg kinematics and a whole-body model, after its cold start
    R.reset(q_des)                        the IK guess of the first tick (srbm_control_tick_reset)
    R.set_state(q, v)                     the plant's (q, v)
    mpc.plant_set_push(time, impulse)     optional: one push per instance
    R.tick_log_enable(200)                optional: one record per tick and instance
    R.advance(0, 200, 50, 1e-3)           200 ticks of 1 ms, an MPC update every 50; asynchronous
    q, v = R.state(); log = R.tick_log()"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)

TICK_LOG_DOUBLES = 64
# one record of the tick log: field name -> slice of its TICK_LOG_DOUBLES doubles (include/srbm_rti.h); [57, 64) is 0
TICK_LOG_FIELDS = dict(tick=0, time=1, targets_status=2, qp_status=3, qp_iters=4, flags=5, base_pose=slice(6, 13), base_twist=slice(13, 19),
                       torques=slice(19, 31), contact_forces=slice(31, 43), contact=slice(43, 47), foot_heights=slice(47, 51), base_accel=slice(51, 57))
FLAG_PUSH, FLAG_UPDATE, FLAG_COAST = 1, 2, 4


def _d(a):
    return a.ctypes.data_as(_dp)


class ControllerRollout:
    def __init__(self, mpc):
        self.mpc, self.L = mpc, mpc.L

    def reset(self, q_des):
        """MPCController's q_des_ for every instance, one q[19] or [batch][19] (srbm_control_tick_reset)"""
        m = self.mpc
        m._chk(self.L.srbm_control_tick_reset(m.h, _d(m._bcast(q_des, 19))))

    def set_state(self, q, v):
        """the plant's configuration q (one [19] or [batch][19]) and velocity v ([18] or [batch][18])"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_state(m.h, _d(m._bcast(q, 19)), _d(m._bcast(v, 18))))

    def state(self):
        """-> q[batch][19], v[batch][18] after the work queued so far"""
        m = self.mpc
        q, v = np.zeros((m.batch, 19)), np.zeros((m.batch, 18))
        m._chk(self.L.srbm_wb_plant_get_state(m.h, _d(q), _d(v)))
        return q, v

    def advance(self, first_tick, ticks, ticks_per_update, tick_dt):
        """ticks first_tick .. first_tick + ticks - 1 of period tick_dt: control tick, plant step, and after every tick k > 0 with
        k % ticks_per_update == 0 an MPC update at k * tick_dt that is in force from tick k + 1; asynchronous on the batch's stream"""
        self.mpc._chk(self.L.srbm_controller_advance(self.mpc.h, int(first_tick), int(ticks), int(ticks_per_update), float(tick_dt)))

    def plant_step_dev(self, tick, tick_dt, q, v, qp_sol, status):
        """the plant step alone on device pointers (ints): q[batch][19], v[batch][18] in place from qp_sol[batch][30], status[batch][2] of
        control_tick_dev; asynchronous, never logs"""
        self.mpc._chk(self.L.srbm_wb_plant_step_dev(self.mpc.h, int(tick), float(tick_dt), q, v, qp_sol, status))

    # ---- the tick log ----
    def tick_log_enable(self, max_ticks):
        """allocate max_ticks x batch records, cursor 0; 0 disables and frees"""
        self.mpc._chk(self.L.srbm_tick_log_enable(self.mpc.h, int(max_ticks)))

    def tick_log_reset(self):
        self.mpc._chk(self.L.srbm_tick_log_reset(self.mpc.h))

    def tick_log_count(self):
        n = C.c_int(0)
        self.mpc._chk(self.L.srbm_tick_log_count(self.mpc.h, C.byref(n)))
        return n.value

    def tick_log(self, first=0, count=None):
        """-> log[count][batch][TICK_LOG_DOUBLES] (synchronous)"""
        count = self.tick_log_count() - first if count is None else count
        a = np.zeros((count, self.mpc.batch, TICK_LOG_DOUBLES))
        self.mpc._chk(self.L.srbm_tick_log_get(self.mpc.h, int(first), int(count), _d(a)))
        return a

    def tick_log_copy_dev(self, ptr, first=0, count=None):
        """device to device on the batch's stream, no synchronisation"""
        count = self.tick_log_count() - first if count is None else count
        self.mpc._chk(self.L.srbm_tick_log_copy_dev(self.mpc.h, int(first), int(count), ptr))
