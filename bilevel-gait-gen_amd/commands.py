"""The command schedule of a whole-controller rollout off the GPU (include/srbm_rti.h, "timed motion commands"; csrc/srbm_command.hiph): builders
of one event from physical values, a schedule for a batch, and the rule itself over a sequence of MPC updates, the same functions the kernel
compiles.  ControllerRollout.set_commands takes what `stack` returns.

    stand = commands.hold(0.0, des12)                                      # the fixed target of srbm_add_quadratic_tracking_cost, as an event
    go = commands.walk(0.5, 0.3, 0.0, mass, des12)                         # from t = 0.5 s: 0.3 m/s in x from where the robot is then
    stop = commands.hold(2.5, des12_there)
    R.set_commands(commands.stack([[stand, go, stop]]))                    # one list for every instance, or one list per instance

One target holds for the whole horizon of an update; `lead` (seconds) moves it ahead along its rate and is the only look-ahead."""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)

MAX_EVENTS, EVENT_DOUBLES, STATE_DOUBLES, RECORD_DOUBLES = 8, 28, 4, 32
FIELDS = dict(t0=0, flags=1, lead=2, reserved=3, des12=slice(4, 16), rate12=slice(16, 28))
RELATIVE = 1                       # bit 0 of the flags: x and y of des12 are offsets from the (x, y) latched at the event's first update
# the tangent state of srbm_add_quadratic_tracking_cost: position, linear momentum, orientation (tangent), angular momentum
POS, MOMENTUM, ORIENTATION, ANGULAR_MOMENTUM = slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12)


def _d(a):
    return a.ctypes.data_as(_dp)


def event(t0, des12, rate12=None, lead=0.0, relative=False):
    """-> event[28]: from t0 on the target is des12 + rate12 * ((t - t0) + lead), plus the latched (x, y) in x and y where `relative`"""
    e = np.zeros(EVENT_DOUBLES)
    e[FIELDS['t0']], e[FIELDS['flags']], e[FIELDS['lead']] = t0, RELATIVE if relative else 0, lead
    e[FIELDS['des12']] = np.asarray(des12, float)
    if rate12 is not None:
        e[FIELDS['rate12']] = np.asarray(rate12, float)
    return e


def hold(t0, des12):
    """-> event[28]: from t0 on the fixed target des12"""
    return event(t0, des12)


def walk(t0, vx, vy, mass, des12, lead=0.0, relative=True):
    """-> event[28]: from t0 on the target moves at (vx, vy) m/s: rates on x and y, mass * vx and mass * vy in the momentum entries of the target,
    the other entries those of des12.  relative (the default): x and y of des12 are offsets from where the robot is at the event's first update"""
    d = np.array(des12, float)
    d[3], d[4] = mass * vx, mass * vy
    rate = np.zeros(12)
    rate[0], rate[1] = vx, vy
    return event(t0, d, rate, lead, relative)


def stack(events_per_instance, batch=None):
    """events_per_instance: one list of events for every instance ([[e0, e1]], with `batch`) or one list per instance, all of one length
    (there is no empty slot: an event that never matters is one whose t0 lies beyond the rollout) -> cmds[batch][n][28]"""
    lists = [list(l) for l in events_per_instance]
    if batch is not None and len(lists) == 1:
        lists = lists * batch
    if batch is not None and len(lists) != batch:
        raise ValueError('one list of events, or one per instance')
    n = len(lists[0])
    if any(len(l) != n for l in lists):
        raise ValueError('every instance has the same number of events')
    if n > MAX_EVENTS:
        raise ValueError('at most %d events per instance' % MAX_EVENTS)
    return np.array(lists, float).reshape(len(lists), n, EVENT_DOUBLES)


def initial_state(batch):
    """-> cstate[batch][4], crec[batch][32] as srbm_controller_set_commands leaves them: nothing latched"""
    cstate, crec = np.zeros((batch, STATE_DOUBLES)), np.zeros((batch, RECORD_DOUBLES))
    cstate[:, 0] = crec[:, 1] = -1.0
    return cstate, crec


def targets(L, cmds, Q, Phi, times, states13, cstate=None, crec=None):
    """the rule on the host (srbm_command_target_host; L: the loaded library, host.lib()): cmds[batch][n][28], Q and Phi [144]-like or
    [batch][144]-like, times[n_updates] or [n_updates][batch], states13[n_updates][batch][13]; cstate / crec: what an earlier call returned (None: nothing
    latched) -> dict(des12, w12, Phi_w12 [n_updates][batch][12] (NaN where no event is in force), in_force[n_updates][batch] (bool), cstate, crec)"""
    c = np.ascontiguousarray(cmds, float)
    if c.ndim != 3 or c.shape[2] != EVENT_DOUBLES:
        raise ValueError('cmds[batch][n_events][28]')
    batch, n = c.shape[:2]
    q = np.ascontiguousarray(np.broadcast_to(np.asarray(Q, float).reshape(-1, 144), (batch, 144)))
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(Phi, float).reshape(-1, 144), (batch, 144)))
    t = np.asarray(times, float)
    t = t[:, None] if t.ndim == 1 else t
    nu = t.shape[0]
    t = np.ascontiguousarray(np.broadcast_to(t, (nu, batch)))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(states13, float), (nu, batch, 13)))
    cs0, cr0 = initial_state(batch)
    cs = cs0 if cstate is None else np.array(cstate, float).reshape(batch, STATE_DOUBLES)
    cr = cr0 if crec is None else np.array(crec, float).reshape(batch, RECORD_DOUBLES)
    des, w, pw = np.zeros((max(nu, 1), batch, 12)), np.zeros((max(nu, 1), batch, 12)), np.zeros((max(nu, 1), batch, 12))
    one = np.zeros(1)
    if L.srbm_command_target_host(n, _d(c if c.size else one), batch, _d(q), _d(p), nu, _d(t if nu else one), _d(s if nu else one), _d(cs), _d(des), _d(w),
                                  _d(pw), _d(cr)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    des, w, pw = des[:nu], w[:nu], pw[:nu]
    return dict(des12=des, w12=w, Phi_w12=pw, in_force=~np.isnan(des[:, :, 0]), cstate=cs, crec=cr)
