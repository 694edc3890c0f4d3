"""The joint model of the torque-driven plant off the GPU (include/srbm_rti.h, "a joint model"; csrc/srbm_wb_joints.hiph): a builder of the per-joint
record from physical values, the A1's values from a fixture keyed by joint name, and the law itself over recorded sub-steps, the same function the
kernels compile.  ControllerRollout.set_joints takes what `record` and `a1_model` return.

    j = joints.record(damping=1.0, armature=0.01, friction=0.2, stiction_band=0.05, q_min=-2.7, q_max=-0.92, motor_time_constant=2e-3)     # one joint
    J, limit = joints.a1_model(json.load(open('tests/golden/a1_joint_model.json')), stiction_band=0.05, motor_time_constant=2e-3)          # [12][8], [12]
    R.set_joints(J, stops=(200.0, 2.0))"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

JOINT_DOUBLES, STOP_DOUBLES, RECORD_DOUBLES = 8, 2, 8
FIELDS = dict(damping=0, armature=1, friction=2, stiction_band=3, q_min=4, q_max=5, motor_time_constant=6)
# this library's joint order (control[0..12), q[7..19)): the legs in foot order, each hip, thigh, calf
JOINT_NAMES = ['%s_%s_joint' % (leg, part) for leg in ('FL', 'FR', 'RL', 'RR') for part in ('hip', 'thigh', 'calf')]


def _d(a):
    return a.ctypes.data_as(_dp)


def record(damping=0.0, armature=0.0, friction=0.0, stiction_band=0.0, q_min=-np.inf, q_max=np.inf, motor_time_constant=0.0):
    """-> joint[8] of one joint; the defaults are the transparent model, under which the plant returns the bytes it returns without the setting"""
    j = np.zeros(JOINT_DOUBLES)
    for k, v in dict(damping=damping, armature=armature, friction=friction, stiction_band=stiction_band, q_min=q_min, q_max=q_max,
                     motor_time_constant=motor_time_constant).items():
        j[FIELDS[k]] = v
    return j


def transparent():
    """-> joints[12][8] of the transparent model"""
    return np.tile(record(), (12, 1))


def a1_model(fixture, stiction_band, motor_time_constant=0.0):
    """the loaded fixture tests/golden/a1_joint_model.json (per joint NAME: damping, armature, frictionloss, range, motor_limit, in the XML's leg
    order FR, FL, RR, RL) -> joints[12][8] in this library's order (JOINT_NAMES: FL, FR, RL, RR), mapped by name, and the motors' torque bounds
    [12] for set_plant.  The fixture has no stiction band (its simulator treats dry friction as a constraint) and no motor lag: the caller chooses"""
    J, lim = np.zeros((12, JOINT_DOUBLES)), np.zeros(12)
    for i, name in enumerate(JOINT_NAMES):
        v = fixture['joints'][name]
        J[i] = record(v['damping'], v['armature'], v['frictionloss'], stiction_band if v['frictionloss'] > 0 else 0.0, v['range'][0], v['range'][1],
                      motor_time_constant)
        lim[i] = v['motor_limit']
    return J, lim


def law(L, h, joints, stops, cmd, off, q_j, v_j, js, jrec=None):
    """the law over recorded sub-steps on the host (srbm_joint_law_host; L: the loaded library, host.lib()): cmd, q_j, v_j [substeps][batch][12] the
    command after its clamp, the joint angles and rates of every sub-step of ONE tick of period h; joints [12][8] or [batch][12][8], stops [2] or
    [batch][2], off [batch] (an instance with its actuators off), js[batch][12] the motor torques before, jrec[batch][8] the record before (None: zero)
    -> tau[substeps][batch][12], the motor torques and the record after (the arguments are not modified)"""
    cmd, q_j, v_j = (np.ascontiguousarray(a, float) for a in (cmd, q_j, v_j))
    if cmd.ndim != 3 or cmd.shape[2] != 12 or q_j.shape != cmd.shape or v_j.shape != cmd.shape:
        raise ValueError('cmd, q_j, v_j [substeps][batch][12]')
    S, batch = cmd.shape[:2]
    joints = np.ascontiguousarray(np.broadcast_to(np.asarray(joints, float), (batch, 12, JOINT_DOUBLES)))
    stops = np.ascontiguousarray(np.broadcast_to(np.asarray(stops, float), (batch, STOP_DOUBLES)))
    off = np.ascontiguousarray(np.broadcast_to(np.asarray(off), (batch,)).astype(np.int32))
    js = np.array(js, float)
    jrec = np.zeros((batch, RECORD_DOUBLES)) if jrec is None else np.array(jrec, float)
    if js.shape != (batch, 12) or jrec.shape != (batch, RECORD_DOUBLES):
        raise ValueError('js[batch][12], jrec[batch][8]')
    tau = np.zeros((S, batch, 12))
    if L.srbm_joint_law_host(batch, S, float(h), _d(joints), _d(stops), _d(cmd), off.ctypes.data_as(_ip), _d(q_j), _d(v_j), _d(js), _d(tau), _d(jrec)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return tau, js, jrec
