"""The MPC period of the closed-loop protocols (include/srbm_rti.h: srbm_plant_set_period, srbm_plant_get_period): the reference's controller
solves at whatever time its state sample carries (controllers/mpc_controller.cpp:299-346), not on the node grid; with a period p set for an instance,
iteration i of srbm_closed_loop_advance / srbm_plant_advance and run i + 1 of srbm_gait_closed_loop_advance integrate its plant from i p over p and
solve at i p + p.  A module of its own beside host.py, as gait_rollout.py and control_tick.py are: it calls through the library `host.declare` has
typed, and tests/test_abi_prototypes.py keeps the method list of host.BatchMPC as it stands.

    plant_set_period(mpc, 0.013)                      one period for the whole batch
    plant_set_period(mpc, [0.05, 0.025, 0.013, ...])  one per instance: a sweep of the MPC rate over one batch
    plant_set_period(mpc)                             back to the node step dt
    plant_period(mpc)                                 period[batch] in effect (dt where none is set)

The open-loop entries (rti_advance, rti_advance_unfused, the gait optimiser's rti_advance) ignore the setting."""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)


def period_array(period, batch):
    """a scalar, or one value per instance, as float64 period[batch]; ValueError on any other shape (before the library is called)"""
    a = np.asarray(period, dtype=np.float64)
    if a.ndim == 0 or a.shape == (1,):
        return np.full(batch, float(a.reshape(())), dtype=np.float64)
    if a.shape != (batch,):
        raise ValueError('period: a scalar or one value per instance (shape (%d,)) expected, got shape %s' % (batch, a.shape))
    return np.ascontiguousarray(a)


def plant_set_period(mpc, period=None):
    """period: seconds, a scalar for the whole batch or period[batch]; None clears (= the node step).  The library refuses a period that is not
    finite, <= 0 or >= num_nodes * dt, naming the instance, and leaves the batch untouched (RuntimeError)"""
    if period is None:
        mpc._chk(mpc.L.srbm_plant_set_period(mpc.h, None))
    else:
        mpc._chk(mpc.L.srbm_plant_set_period(mpc.h, period_array(period, mpc.batch).ctypes.data_as(_dp)))


def plant_period(mpc):
    """period[batch] in effect: the value set for each instance, the node step dt where none is set"""
    out = np.zeros(mpc.batch)
    mpc._chk(mpc.L.srbm_plant_get_period(mpc.h, out.ctypes.data_as(_dp)))
    return out
