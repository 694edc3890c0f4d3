"""The sensor model of whole-controller rollouts off the GPU (include/srbm_rti.h, "sensor model"; csrc/srbm_sensors.hiph): a builder of the per-instance
record from physical values, and the entries that need no GPU -- one Philox4x32-10 block, the sensor state of a plant at (q, v), and the model itself
over a recorded sequence of true states, the same function the kernel compiles.  ControllerRollout.set_sensors takes what `record` returns.

    sens = sensors.record(mocap_ticks=5, sigma_p=1e-3, sigma_r=2e-3, velocity_source=1, sigma_w=0.01, gyro_bias=(0.01, 0, -0.01),
                          sigma_qj=1e-3, sigma_vj=0.05, lpf_base=sensors.lpf_x(40.0, 1e-3), lpf_joints=sensors.lpf_x(100.0, 1e-3))
    R.set_sensors(sens, seed=np.arange(batch))"""
import ctypes as C
import math

import numpy as np

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_llp = C.POINTER(C.c_longlong)

SENSOR_DOUBLES, STATE_DOUBLES, RECORD_DOUBLES = 16, 72, 8
FIELDS = dict(mocap_ticks=0, mocap_delay=1, sigma_p=2, sigma_r=3, velocity_source=4, sigma_v=5, sigma_w=6, gyro_bias=slice(7, 10), sigma_qj=10, sigma_vj=11,
              lpf_base=12, lpf_joints=13)
VELOCITY_FROM_PLANT, VELOCITY_FROM_MOCAP = 0, 1


def _d(a):
    return a.ctypes.data_as(_dp)


def lpf_x(fpass, tick_dt):
    """the x of the reference's first-order low-pass filter (hardware_robot.cpp:676-679) for a pass frequency in Hz at one step per tick"""
    return math.tan(math.pi * fpass * tick_dt)


def record(mocap_ticks=1, mocap_delay=0, sigma_p=0.0, sigma_r=0.0, velocity_source=VELOCITY_FROM_PLANT, sigma_v=0.0, sigma_w=0.0, gyro_bias=(0.0, 0.0, 0.0),
           sigma_qj=0.0, sigma_vj=0.0, lpf_base=0.0, lpf_joints=0.0):
    """-> sens[16] of one instance; the defaults are the transparent model, whose measurement is the bytes of the state"""
    s = np.zeros(SENSOR_DOUBLES)
    for k, v in dict(mocap_ticks=mocap_ticks, mocap_delay=mocap_delay, sigma_p=sigma_p, sigma_r=sigma_r, velocity_source=velocity_source, sigma_v=sigma_v,
                     sigma_w=sigma_w, gyro_bias=gyro_bias, sigma_qj=sigma_qj, sigma_vj=sigma_vj, lpf_base=lpf_base, lpf_joints=lpf_joints).items():
        s[FIELDS[k]] = v
    return s


def _chk(L, rc):
    if rc != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())


def _seeds(seed, batch):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64), (batch,))).view(np.int64)


def philox(L, counter, key):
    """one Philox4x32-10 block on the host (srbm_sensor_philox_host; L: the loaded library, host.lib()): counter[4], key[2] -> out[4], uint32"""
    c, k, o = np.ascontiguousarray(counter, np.uint32), np.ascontiguousarray(key, np.uint32), np.zeros(4, np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError('counter[4], key[2]')
    _chk(L, L.srbm_sensor_philox_host(c.view(np.int32).ctypes.data_as(_ip), k.view(np.int32).ctypes.data_as(_ip), o.view(np.int32).ctypes.data_as(_ip)))
    return o


def state_init(L, q, v):
    """-> ms[batch][72]: no sample taken, the ring full of the pose of q, the filters at rest on v (srbm_sensor_state_init_host)"""
    q, v = np.ascontiguousarray(q, float), np.ascontiguousarray(v, float)
    if q.ndim != 2 or q.shape[1] != 19 or v.shape != (len(q), 18):
        raise ValueError('q[batch][19], v[batch][18]')
    ms = np.zeros((len(q), STATE_DOUBLES))
    _chk(L, L.srbm_sensor_state_init_host(len(q), _d(q), _d(v), _d(ms)))
    return ms


def measure(L, first_tick, tick_dt, sens, seed, q_true, v_true, ms, srec=None):
    """the model over a recorded sequence on the host (srbm_sensor_measure_host): q_true[ticks][batch][19], v_true[ticks][batch][18] of ticks
    first_tick .. first_tick + ticks - 1, ms[batch][72] the sensor state before, srec[batch][8] the record before (None: zero)
    -> qm[ticks][batch][19], vm[ticks][batch][18], the state and the record after (the arguments are not modified)"""
    q_true, v_true = np.ascontiguousarray(q_true, float), np.ascontiguousarray(v_true, float)
    if q_true.ndim != 3 or q_true.shape[2] != 19 or v_true.shape != q_true.shape[:2] + (18,):
        raise ValueError('q_true[ticks][batch][19], v_true[ticks][batch][18]')
    ticks, batch = q_true.shape[:2]
    sens = np.ascontiguousarray(np.broadcast_to(np.asarray(sens, float), (batch, SENSOR_DOUBLES)))
    ms = np.array(ms, float)
    srec = np.zeros((batch, RECORD_DOUBLES)) if srec is None else np.array(srec, float)
    if ms.shape != (batch, STATE_DOUBLES) or srec.shape != (batch, RECORD_DOUBLES):
        raise ValueError('ms[batch][72], srec[batch][8]')
    qm, vm = np.zeros((max(ticks, 1), batch, 19)), np.zeros((max(ticks, 1), batch, 18))
    one = np.zeros(1)
    _chk(L, L.srbm_sensor_measure_host(batch, int(first_tick), ticks, float(tick_dt), _d(sens), _seeds(seed, batch).ctypes.data_as(_llp),
                                       _d(q_true if ticks else one), _d(v_true if ticks else one), _d(ms), _d(srec), _d(qm), _d(vm)))
    return qm[:ticks], vm[:ticks], ms, srec
