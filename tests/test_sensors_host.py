"""The sensor model of whole-controller rollouts on the host (no GPU): srbm_sensor_philox_host, srbm_sensor_state_init_host and
srbm_sensor_measure_host through srbm_loader.sensors against the restatement of tests/sensors_kit.py, written from the tables of include/srbm_rti.h.
srbm_sensor_measure_host compiles the function the kernel srbm_k_measure compiles (csrc/srbm_sensors.hiph), one component of the measurement at a
time; the kit goes per instance and per quantity in np.float64 scalars.  Every comparison is bitwise: the model uses + - * / only, one rounded
operation per statement, the quaternion product, its first-order normalisation and the rotation included, and IEEE division rounds alike in the
compiled code and in numpy -- no component needed the 4 ulp allowance."""
import numpy as np
import pytest

import sensors_kit as sk
from srbm_loader import host, sensors

H = 0.01
TICKS = 40


@pytest.fixture(scope='module')
def L():
    host.build()
    return host.lib()


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        raise AssertionError('%s: %d of %d values differ, first at %s: %r against %r' % (what, len(bad), a.size, bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def unit(q):
    return q / np.linalg.norm(q)


def synthetic(ticks=TICKS, batch=4, seed=3):
    """a smooth sequence of true states: a base that moves and turns, joints that swing"""
    rng = np.random.default_rng(seed)
    q, v = np.zeros((ticks, batch, 19)), np.zeros((ticks, batch, 18))
    ph = rng.uniform(0, 6, size=(batch, 19))
    for k in range(ticks):
        t = k * H
        for b in range(batch):
            q[k, b, :3] = [0.3 * t + 0.01 * b, 0.1 * np.sin(3 * t + ph[b, 0]), 0.3 + 0.02 * np.cos(5 * t + ph[b, 1])]
            ang = np.array([0.1 * np.sin(4 * t + ph[b, 2]), 0.15 * np.cos(3 * t + ph[b, 3]), 0.4 * t + 0.2 * b])
            half = 0.5 * np.linalg.norm(ang)
            q[k, b, 3:7] = unit(np.concatenate([np.sin(half) * ang / (2 * half), [np.cos(half)]]))
            q[k, b, 7:] = 0.5 * np.sin(6 * t + ph[b, 7:])
            v[k, b] = np.concatenate([[0.3, 0.3 * np.cos(3 * t), -0.1 * np.sin(5 * t)], 0.5 * np.cos(4 * t + ph[b, 3:6]), 3.0 * np.cos(6 * t + ph[b, 7:])])
    return q, v


KNOWN = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]


@pytest.mark.parametrize('counter,key,want', KNOWN)
def test_philox_known_answers(L, counter, key, want):
    want = [int(w, 16) for w in want.split()]
    assert sk.philox(counter, key) == want
    assert sensors.philox(L, counter, key).tolist() == want


def test_noise_statistics(L):
    seed, ch = 7 + 2 ** 32, 3
    z = np.array([sk.unit_noise(seed, k, ch) for k in range(20000)])
    print('mean %.4f std %.4f range %.2f .. %.2f' % (z.mean(), z.std(), z.min(), z.max()))
    assert abs(z.mean()) <= 0.03 and abs(z.std() - 1.0) <= 0.02 and np.abs(z).max() <= 2 * np.sqrt(3.0)
    # ... and the library's draw is the kit's: a position channel with sigma 1 on a zero state is z itself
    q, v = np.zeros((50, 1, 19)), np.zeros((50, 1, 18))
    q[:, :, 6] = 1.0
    qm, _, _, _ = sensors.measure(L, 0, H, sensors.record(sigma_r=0.0, sigma_p=1.0), seed, q, v, sensors.state_init(L, q[0], v[0]))
    same_bytes(qm[:, 0, 0], [sk.unit_noise(seed, k, 0) for k in range(50)], 'position noise of sigma 1')


def test_the_transparent_model_copies_bytes(L):
    q, v = synthetic()
    q[3, 1, 8], v[5, 2, 4], v[6, 0, 1] = -0.0, -0.0, -0.0          # (a sum with a zero bias or a zero noise would turn these into +0)
    ms0 = sensors.state_init(L, q[0], v[0])
    qm, vm, ms, srec = sensors.measure(L, 0, H, sensors.record(), [1, 2, 3, 4], q, v, ms0)
    same_bytes(qm, q, 'qm against q')
    same_bytes(vm, v, 'vm against v')
    same_bytes(srec, np.array([[TICKS, TICKS, 0, 0, 0, 0, 0, 0]] * 4, float), 'record')
    assert ms[:, 0].tolist() == [TICKS] * 4
    same_bytes(ms[:, 54:], v[-1], 'filter memory')


def test_state_init(L):
    q, v = synthetic(1)
    ms = sensors.state_init(L, q[0], v[0])
    same_bytes(ms, np.array([sk.state_init(q[0, b], v[0, b]) for b in range(4)]), 'state')
    assert ms.shape == (4, sensors.STATE_DOUBLES) and np.all(ms[:, 0] == 0)
    for s in range(5):
        same_bytes(ms[:, 1 + 7 * s:8 + 7 * s], q[0, :, :7], 'ring slot %d' % s)


def test_against_the_restatement_and_cut(L):
    """bitwise on every component, the state and the record included; 40 ticks in one call are 13 + 27"""
    sens, seed = sk.four_instances(H, sensors.record, sensors.lpf_x)
    assert sens[:, 0].tolist() == [1, 2, 3, 5] and sens[:, 1].tolist() == [0, 1, 2, 3] and sens[:, 4].tolist() == [0, 1, 0, 1]
    assert (sens[:, 12:14] != 0).tolist() == [[True, True], [False, True], [False, False], [True, False]]
    assert not sens[2, [2, 3, 5, 6, 10, 11]].any() and sens[2, 7:10].any()
    q, v = synthetic()
    ms0 = sensors.state_init(L, q[0], v[0])
    got = sensors.measure(L, 0, H, sens, seed, q, v, ms0)
    want = sk.measure(0, H, sens, seed, q, v, ms0)
    for g, w, name in zip(got, want, ('qm', 'vm', 'sensor state', 'sensor record')):
        same_bytes(g, w, name)
    qm, vm, ms, srec = got
    assert srec[:, 0].tolist() == [40] * 4 and srec[:, 1].tolist() == [40, 20, 14, 8] and ms[:, 0].tolist() == [40, 20, 14, 8]
    assert np.all(srec[[0, 1, 3], 2] > 0) and srec[2, 2] > 0          # (instance 2: no noise, but its pose is two samples of three ticks old)
    # instance 2, a gyro bias only: joints, linear velocity and joint rates are the truth; the gyro is off by the bias
    same_bytes(qm[:, 2, 7:], q[:, 2, 7:], 'instance 2: joint angles')
    same_bytes(vm[:, 2, :3], v[:, 2, :3], 'instance 2: linear velocity')
    same_bytes(vm[:, 2, 6:], v[:, 2, 6:], 'instance 2: joint rates')
    same_bytes(vm[:, 2, 3], v[:, 2, 3] + 0.02, 'instance 2: gyro x')
    same_bytes(vm[:, 2, 4], v[:, 2, 4], 'instance 2: gyro y (bias 0)')
    # the delay: instance 2 at tick 9 has samples of ticks 0, 3, 6, 9 and reads the one of tick 3
    same_bytes(qm[9, 2, :7], q[3, 2, :7], 'instance 2: the pose two samples behind')
    same_bytes(qm[5, 2, :7], q[0, 2, :7], 'instance 2: the pre-fill')
    # the cut
    a = sensors.measure(L, 0, H, sens, seed, q[:13], v[:13], ms0)
    b = sensors.measure(L, 13, H, sens, seed, q[13:], v[13:], a[2], a[3])
    same_bytes(np.concatenate([a[0], b[0]]), qm, 'qm of 13 + 27')
    same_bytes(np.concatenate([a[1], b[1]]), vm, 'vm of 13 + 27')
    same_bytes(b[2], ms, 'state of 13 + 27')
    same_bytes(b[3], srec, 'record of 13 + 27')


def test_the_finite_difference_is_the_body_velocity(L):
    yaw, vw, mt, delay = 0.7, np.array([0.4, -0.25, 0.1]), 3, 1
    qt = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])
    R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    q, v = np.zeros((TICKS, 1, 19)), np.zeros((TICKS, 1, 18))
    for k in range(TICKS):
        q[k, 0, :3], q[k, 0, 3:7] = np.array([1.0, 2.0, 0.3]) + vw * (k * H), qt
    qm, vm, ms, srec = sensors.measure(L, 0, H, sensors.record(mocap_ticks=mt, mocap_delay=delay, velocity_source=1), 9, q, v, sensors.state_init(L, q[0], v[0]))
    real = (delay + 2 - 1) * mt          # the tick on which the sample behind the available one is the first real one
    assert np.all(vm[:delay * mt, 0, :3] == 0)          # the two entries are the pre-fill
    err = np.abs(vm[real:, 0, :3] - R.T @ vw).max()
    print('finite difference against R\' v_world: %.2e' % err)
    assert err <= 1e-12
    assert srec[0, 4] >= np.abs(R.T @ vw).max() - 1e-12          # (the true v of this sequence is 0: the record holds the difference)


def test_refusals_name_instance_and_field(L):
    q, v = synthetic(2)
    ms0 = sensors.state_init(L, q[0], v[0])
    ok = np.array([sensors.record()] * 4)
    cases = [((1, 0), 0.0, 'instance 1: mocap_ticks'), ((1, 0), 2.5, 'instance 1: mocap_ticks'), ((0, 0), 65, 'instance 0: mocap_ticks'),
             ((2, 1), 4, 'instance 2: mocap_delay'), ((2, 1), -1, 'instance 2: mocap_delay'), ((3, 1), 0.5, 'instance 3: mocap_delay'),
             ((0, 2), -1e-3, 'instance 0: sigma_p'), ((1, 3), np.nan, 'instance 1: sigma_r'), ((2, 4), 2, 'instance 2: velocity_source'),
             ((3, 5), -1.0, 'instance 3: sigma_v'), ((0, 6), np.inf, 'instance 0: sigma_w'), ((1, 8), np.nan, r'instance 1: gyro_bias\[1\]'),
             ((2, 10), -2.0, 'instance 2: sigma_qj'), ((3, 11), -np.inf, 'instance 3: sigma_vj'), ((0, 12), -0.1, 'instance 0: lpf_x_base'),
             ((1, 13), -0.1, 'instance 1: lpf_x_joints'), ((2, 14), 1.0, r'instance 2: reserved\[14\]'), ((3, 15), -1.0, r'instance 3: reserved\[15\]')]
    for (b, f), bad, msg in cases:
        sens = ok.copy()
        sens[b, f] = bad
        with pytest.raises(RuntimeError, match=msg):
            sensors.measure(L, 0, H, sens, 0, q, v, ms0)
    sens = ok.copy()
    sens[1, 7:10] = [-0.5, 0.0, 0.5]          # a negative bias is a bias
    sensors.measure(L, 0, H, sens, 0, q, v, ms0)
    for args, msg in (((-1, H), 'first_tick'), ((0, 0.0), 'tick_dt'), ((0, np.nan), 'tick_dt')):
        with pytest.raises(RuntimeError, match=msg):
            sensors.measure(L, args[0], args[1], ok, 0, q, v, ms0)
    assert sensors.lpf_x(25.0, 1e-3) == np.tan(np.pi * 25.0 * 1e-3)
