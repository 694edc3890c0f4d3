"""The wrench schedule of the torque-driven plant off the GPU (include/srbm_rti.h, "timed external wrenches"; csrc/srbm_wb_wrench.hiph): a builder
of one event from physical values with the body taken by name, a schedule padded with empty slots, and the activity rule itself over the sub-steps
of a rollout, the same function the kernels compile.  ControllerRollout.set_wrenches takes what `schedule` returns.

    shove = wrenches.event(0.5, 0.15, 'trunk', force=(0, 60, 0))                                 # 60 N held for 150 ms
    kick = wrenches.event(1.0, 0.01, 'FL_calf', point=(0, 0, -0.1), force=(80, 0, 0))            # a kick on a shank
    load = wrenches.event(2.0, float('inf'), 'trunk', point=(-0.1, 0, 0.05), force=(0, 0, -49.05))   # 5 kg dropped on the back at t = 2 s
    R.set_wrenches(wrenches.schedule(batch, [[shove, kick, load]]))"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

EVENTS, EVENT_DOUBLES, RECORD_DOUBLES = 8, 16, 8
FIELDS = dict(t0=0, duration=1, body=2, frame=3, point=slice(4, 7), force=slice(7, 10), torque=slice(10, 13))
FRAMES = dict(world=0, body=1)
# SrbmWbcParams::body order: the trunk, then the legs in foot order, each hip, thigh, calf
BODY_NAMES = ['trunk'] + ['%s_%s' % (leg, part) for leg in ('FL', 'FR', 'RL', 'RR') for part in ('hip', 'thigh', 'calf')]


def _d(a):
    return a.ctypes.data_as(_dp)


def event(t0, duration, body, point=(0, 0, 0), force=(0, 0, 0), torque=(0, 0, 0), frame='world'):
    """-> event[16]: from t0 for `duration` seconds (inf: for good; 0 makes an empty slot) on `body` (a name of BODY_NAMES or its index 0..12), at
    `point` in the body's joint frame, force and torque in `frame` axes ('world', or 'body': they turn with the body)"""
    e = np.zeros(EVENT_DOUBLES)
    e[FIELDS['t0']], e[FIELDS['duration']] = t0, duration
    e[FIELDS['body']] = BODY_NAMES.index(body) if isinstance(body, str) else body
    e[FIELDS['frame']] = FRAMES[frame] if isinstance(frame, str) else frame
    e[FIELDS['point']], e[FIELDS['force']], e[FIELDS['torque']] = point, force, torque
    return e


def empty():
    """-> event[16] that never acts (d = 0)"""
    return np.zeros(EVENT_DOUBLES)


def schedule(batch, events_per_instance):
    """events_per_instance: one list of events for every instance ([[e0, e1]]) or `batch` lists -> wrenches[batch][n][16], n the longest list
    (at least 1), the shorter ones padded with empty slots"""
    lists = [list(l) for l in events_per_instance]
    if len(lists) == 1:
        lists = lists * batch
    if len(lists) != batch:
        raise ValueError('one list of events, or one per instance')
    n = max(1, max(len(l) for l in lists))
    if n > EVENTS:
        raise ValueError('at most %d events per instance' % EVENTS)
    w = np.zeros((batch, n, EVENT_DOUBLES))
    for b, l in enumerate(lists):
        for i, e in enumerate(l):
            w[b, i] = e
    return w


def active(L, wrenches, first_tick, ticks, tick_dt, substeps):
    """the activity rule on the host (srbm_wrench_active_host; L: the loaded library, host.lib()): wrenches[batch][n][16]
    -> mask[ticks][substeps][batch] (int32, bit e: event e is active in that sub-step) of ticks first_tick .. first_tick + ticks - 1"""
    w = np.ascontiguousarray(wrenches, float)
    if w.ndim != 3 or w.shape[2] != EVENT_DOUBLES:
        raise ValueError('wrenches[batch][n_events][16]')
    batch, n = w.shape[:2]
    mask = np.zeros((max(ticks, 1), max(substeps, 1), batch), np.int32)
    if L.srbm_wrench_active_host(n, _d(w if w.size else np.zeros(1)), batch, int(first_tick), int(ticks), float(tick_dt), int(substeps), mask.ctypes.data_as(_ip)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return mask[:ticks]
