"""The sensor model of whole-controller rollouts on the GPU (srbm_controller_set_sensors, csrc/srbm_sensors.hiph, through
ControllerRollout.set_sensors / sensors / sensor_state / set_sensor_state / sensor_record / measured / measure_dev): with sensors set the control
ticks read a measurement (qm, vm) of the plant's (q, v) -- a mocap pose at its own rate and delay, a finite-difference or noisy linear velocity, a
biased gyro, noisy joints, low-pass filters -- while the plant, the push, the ground and the tick-log head keep the truth.

    1  the transparent model is no model, byte for byte, on plant kind 0 and on the ground;
    2  the kernel alone, on both builds, against srbm_sensor_measure_host on the same inputs: bitwise, state and record included;
    3  what the controller reads is the measurement: one call, one call per tick and the host-driven chain;
    4  the tick log holds the truth;
    5  instances are independent;
    6  a rollout cut at tick 7 and continued is the same rollout;
    7  clone, set_state, set_sensors(None), refusals;
    8  on the raised ground with contact feedback, a latency and the gait step: one call against one call per tick.

The shapes of tests/controller_rollout_kit.py: 4 Config-B instances, ticks of 10 ms, an update every 5, 12 ticks.  The four instances of
sensors_kit.four_instances: mocap_ticks 1 / 2 / 3 / 5, delays 0..3, both velocity sources, filters on and off, instance 2 with a gyro bias only."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
import sensors_kit as sk
from gpu_kit import same_bytes
from srbm_loader import host, sensors
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS as F, SENSOR_RECORD_FIELDS as SR
from test_gpu_controller_rollout import World, Dev, assert_same          # the batch of the rollout tests and its helpers

pytestmark = pytest.mark.gpu
B, H, TPU, N = kit.B, kit.TICK_DT, kit.TPU, 12
SENS, SEED = sk.four_instances(H, sensors.record, sensors.lpf_x)
TRANSPARENT = sensors.record()


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def plain(world):
    """the rollout without the setting: its end, its logs and the plant's state before every tick (one call per tick; read only)"""
    g, R = world.fresh(tick_log=N, step_log=4)
    q, v = [], []
    for k in range(N):
        qk, vk = R.state()
        q.append(qk); v.append(vk)
        R.advance(k, 1, TPU, H)
    return dict(end=snap(g, R, N, sens=False), tick_log=R.tick_log(), step_log=g.step_log(), q=np.array(q), v=np.array(v))


def traj_bytes(arr):
    return np.frombuffer(bytes(arr), np.uint8)


def snap(g, R, next_tick, sens=True, q=None, v=None):
    """what a rollout leaves behind (test_gpu_controller_rollout.snapshot) and, with sensors set, the sensor state, the record and the last measurement"""
    if q is None:
        q, v = R.state()
    probe = ControlTick(g.clone()).tick(q, v, next_tick * H)
    s = dict(q=q, v=v, trajectory=traj_bytes(g.get_trajectory()), q_des=probe['q_des'], probe_sol=probe['qp_sol'])
    if sens:
        s['sensor_state'], s['sensor_record'] = R.sensor_state(), R.sensor_record()
        s['qm'], s['vm'] = R.measured()
    return s


def test_the_transparent_model_is_no_model(world, plain):
    g, R = world.fresh(tick_log=N, step_log=4)
    R.set_sensors(TRANSPARENT, SEED)
    R.advance(0, N, TPU, H)
    assert_same(plain['end'], snap(g, R, N, sens=False), 'transparent sensors against none')
    same_bytes(R.tick_log(), plain['tick_log'], 'tick log')
    same_bytes(g.step_log(), plain['step_log'], 'step log')
    assert g.step_log_count() == 2
    qm, vm = R.measured()
    same_bytes(qm, plain['q'][N - 1], 'the last measurement against the plant before the last tick')
    same_bytes(vm, plain['v'][N - 1], 'the last measurement against the plant before the last tick (v)')
    same_bytes(R.sensor_record(), np.array([[N, N, 0, 0, 0, 0, 0, 0]] * B, float), 'record')


def test_the_transparent_model_is_no_model_on_the_ground(world):
    gw, k0 = ck.GroundWorld(world), 20
    ground = ck.flat_ground(gw, k0)
    runs = []
    for sens in (None, TRANSPARENT):
        g, R = gw.fresh(k0, ground, tick_log=N, step_log=4)
        if sens is not None:
            R.set_sensors(sens, SEED)
        R.advance(k0, N, TPU, H)
        s = snap(g, R, k0 + N, sens=False)
        s['cs'], s['tick_log'], s['step_log'] = R.contact_state(), R.tick_log(), g.step_log()
        runs.append(s)
    assert_same(runs[0], runs[1], 'transparent sensors against none, on the ground')
    assert runs[0]['tick_log'][:, :, 57].min() == 1 and runs[0]['tick_log'][:, :, 63].min() >= 4096          # the torque-driven plant on its ground


@pytest.mark.parametrize('large', [False, True], ids=['standard', 'large'])
def test_the_kernel_alone(world, plain, large):
    w = world
    g = host.BatchMPC.cold_start(w.cfg, w.states, w.ees, large=large)
    R = ControllerRollout(g)
    with pytest.raises(RuntimeError, match='no sensors are set'):
        R.measure_dev(0, H, 1, 2, 3, 4)
    R.set_sensors(SENS, SEED)          # (before a plant state: the sensor state starts when it is set)
    with pytest.raises(RuntimeError, match="the plant's state is not"):
        R.measure_dev(0, H, 1, 2, 3, 4)
    R.set_state(plain['q'][0], plain['v'][0])
    ms0 = R.sensor_state()
    same_bytes(ms0, sensors.state_init(g.L, plain['q'][0], plain['v'][0]), 'sensor state at set_state')
    dq, dv, dqm, dvm = Dev(plain['q'][0]), Dev(plain['v'][0]), Dev(np.zeros((B, 19))), Dev(np.zeros((B, 18)))
    with pytest.raises(RuntimeError, match='must not be written over'):
        R.measure_dev(0, H, dq.p.value, dv.p.value, dq.p.value, dvm.p.value)
    with pytest.raises(RuntimeError, match='tick >= 0'):
        R.measure_dev(-1, H, dq.p.value, dv.p.value, dqm.p.value, dvm.p.value)
    qm, vm = [], []
    for k in range(N):
        g.synchronize()
        dq.put(plain['q'][k]); dv.put(plain['v'][k])
        R.measure_dev(k, H, dq.p.value, dv.p.value, dqm.p.value, dvm.p.value)
        g.synchronize()
        qm.append(dqm.get()); vm.append(dvm.get())
    want_qm, want_vm, want_ms, want_rec = sensors.measure(g.L, 0, H, SENS, SEED, plain['q'], plain['v'], ms0)
    same_bytes(np.array(qm), want_qm, 'qm: the kernel against the host')
    same_bytes(np.array(vm), want_vm, 'vm: the kernel against the host')
    same_bytes(R.sensor_state(), want_ms, 'sensor state')
    same_bytes(R.sensor_record(), want_rec, 'sensor record')
    same_bytes(dq.get(), plain['q'][N - 1], 'the true state is only read')
    rec = R.sensor_record()
    assert rec[:, SR['ticks']].tolist() == [N] * B and rec[:, SR['samples']].tolist() == [12, 6, 4, 3]
    assert np.all(rec[[0, 1, 3], SR['max_position']] > 0) and rec[2, SR['max_angular_velocity']] == pytest.approx(0.03, abs=1e-12)
    assert rec[2, SR['max_joint_angle']] == 0 and rec[2, SR['max_joint_rate']] == 0 and rec[2, SR['max_linear_velocity']] == 0
    s, sd = R.sensors()
    same_bytes(s, SENS, 'the setting back')
    assert sd.tolist() == SEED.tolist()
    g.close()


def run_chain(g, R, q, v, first, ticks, tpu):
    """the loop driven from the host: srbm_controller_measure_dev on the true (q, v), srbm_control_tick_dev on (qm, vm), srbm_wb_plant_step_dev on the
    true state, srbm_get_real_time_update_dev on the state and ee the tick wrote.  -> the final (q, v), and (qm, vm) of every tick"""
    T = ControlTick(g)
    n = g.batch
    d = dict(q=Dev(q), v=Dev(v), qm=Dev(np.zeros((n, 19))), vm=Dev(np.zeros((n, 18))), t=Dev(np.zeros(n)), control=Dev(np.zeros((n, 36))),
             qp_sol=Dev(np.zeros((n, 30))), status=Dev(np.zeros((n, 2), np.int32)), contact=Dev(np.zeros((n, 4), np.int32)), state=Dev(np.zeros((n, 13))),
             ee=Dev(np.zeros((n, 4, 3))))
    p = {k: x.p.value for k, x in d.items()}
    measured = []
    for k in range(first, first + ticks):
        g.synchronize()
        d['t'].put(np.full(n, k * H))
        R.measure_dev(k, H, p['q'], p['v'], p['qm'], p['vm'])
        T.tick_dev(p['qm'], p['vm'], p['t'], p['control'], p['qp_sol'], p['status'], None, None, p['contact'], p['state'], p['ee'])
        R.plant_step_dev(k, H, p['q'], p['v'], p['qp_sol'], p['status'])
        if k > 0 and k % tpu == 0:
            g.get_real_time_update_dev(p['state'], p['t'], p['ee'])
        g.synchronize()
        measured.append((d['qm'].get(), d['vm'].get()))
    return d['q'].get(), d['v'].get(), measured


def test_what_the_controller_reads_is_the_measurement(world, plain):
    w = world
    ga, Ra = w.fresh(tick_log=N, step_log=4)
    Ra.set_sensors(SENS, SEED)
    Ra.advance(0, N, TPU, H)
    gb, Rb = w.fresh(tick_log=N, step_log=4)
    Rb.set_sensors(SENS, SEED)
    per_tick = []
    for k in range(N):
        Rb.advance(k, 1, TPU, H)
        per_tick.append(Rb.measured())
    gc, Rc = w.fresh(step_log=4)
    Rc.set_sensors(SENS, SEED)
    qc, vc, chain = run_chain(gc, Rc, w.q, w.v, 0, N, TPU)
    sa = snap(ga, Ra, N)
    assert_same(sa, snap(gb, Rb, N), 'one call per tick against one call')
    sc = snap(gc, Rc, N, q=qc, v=vc)
    sc['qm'], sc['vm'] = chain[-1]          # (the chain measured into its own arrays)
    assert_same(sa, sc, 'the host-driven chain against one call')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log: one call per tick')
    same_bytes(ga.step_log(), gb.step_log(), 'step log: one call per tick')
    same_bytes(ga.step_log(), gc.step_log(), 'step log: the chain')
    for k in range(N):
        same_bytes(per_tick[k][0], chain[k][0], 'qm of tick %d: the entry against the chain' % k)
        same_bytes(per_tick[k][1], chain[k][1], 'vm of tick %d: the entry against the chain' % k)
    # the measurement did something: another rollout than without it, for every instance
    for b in range(B):
        assert Ra.tick_log()[:, b].tobytes() != plain['tick_log'][:, b].tobytes(), b
    assert sa['trajectory'].tobytes() != plain['end']['trajectory'].tobytes()


def test_the_tick_log_holds_the_truth(world):
    g, R = world.fresh(tick_log=N)
    R.set_sensors(SENS, SEED)
    for k in range(N):
        q, v = R.state()
        R.advance(k, 1, TPU, H)
        rec = R.tick_log(k, 1)[0]
        same_bytes(rec[:, F['base_pose']], q[:, :7], 'tick %d: fields 6..12 against the plant before the tick' % k)
        same_bytes(rec[:, F['base_twist']], v[:, :6], 'tick %d: fields 13..18 against the plant before the tick' % k)
        qm, vm = R.measured()
        # sigma_p > 0: instance 0 reads this tick's noisy sample; 1 and 3 read delayed ones, at tick 0 the pre-fill, which is the truth of tick 0
        for b in (0, 1, 3) if k > 0 else (0,):
            assert not np.array_equal(rec[b, F['base_pose']][:3], qm[b, :3]), (k, b)


def test_instances_are_independent(world, plain):
    sens = np.array([TRANSPARENT] * B)
    sens[2] = sensors.record(gyro_bias=(0.05, -0.04, 0.03))
    g, R = world.fresh(tick_log=N, step_log=4)
    R.set_sensors(sens, SEED)
    R.advance(0, N, TPU, H)
    s = snap(g, R, N, sens=False)
    log, trajs, plain_trajs = R.tick_log(), s['trajectory'].reshape(B, -1), plain['end']['trajectory'].reshape(B, -1)
    for b in (0, 1, 3):
        same_bytes(log[:, b], plain['tick_log'][:, b], 'tick log of instance %d' % b)
        same_bytes(trajs[b], plain_trajs[b], 'trajectory of instance %d' % b)
        for key in ('q', 'v', 'q_des', 'probe_sol'):
            same_bytes(s[key][b], plain['end'][key][b], '%s of instance %d' % (key, b))
    assert log[0, 2].tobytes() != plain['tick_log'][0, 2].tobytes() and trajs[2].tobytes() != plain_trajs[2].tobytes()
    # ... its trajectory moves with the first update, which starts from the state the tick reconstructed from the biased gyro
    g2, R2 = world.fresh()
    R2.set_sensors(sens, SEED)
    R2.advance(0, TPU + 1, TPU, H)
    g3, R3 = world.fresh()
    R3.advance(0, TPU + 1, TPU, H)
    t2, t3 = traj_bytes(g2.get_trajectory()).reshape(B, -1), traj_bytes(g3.get_trajectory()).reshape(B, -1)
    assert [t2[b].tobytes() == t3[b].tobytes() for b in range(B)] == [True, True, False, True]
    err = R.sensor_record()[:, SR['max_angular_velocity']]
    assert err[[0, 1, 3]].tolist() == [0, 0, 0] and abs(err[2] - 0.05) <= 1e-12          # (fl(w + b) - w is the bias to rounding)


def test_cut_and_continue(world):
    ga, Ra = world.fresh(tick_log=N, step_log=4)
    Ra.set_sensors(SENS, SEED)
    Ra.advance(0, N, TPU, H)
    gb, Rb = world.fresh(tick_log=N, step_log=4)
    Rb.set_sensors(SENS, SEED)
    Rb.advance(0, 7, TPU, H)
    assert Rb.sensor_record()[:, SR['samples']].tolist() == [7, 4, 3, 2]
    Rb.advance(7, N - 7, TPU, H)
    assert_same(snap(ga, Ra, N), snap(gb, Rb, N), 'the cut rollout against one call')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')


def test_clone_reset_refusals(world, plain):
    w = world
    g, R = w.fresh(step_log=4)
    R.set_sensors(SENS, SEED)
    R.advance(0, 7, TPU, H)
    c = g.clone()
    Rc = ControllerRollout(c)
    assert_same(snap(g, R, 7), snap(c, Rc, 7), 'the clone')
    same_bytes(Rc.sensors()[0], SENS, 'the clone: the setting')
    assert Rc.sensors()[1].tolist() == SEED.tolist()
    R.advance(7, 5, TPU, H)
    Rc.advance(7, 5, TPU, H)
    s = snap(g, R, N)
    assert_same(s, snap(c, Rc, N), 'the clone, 5 ticks on')
    # the state round trip: what get returns, set, leaves the same continuation
    d = g.clone()
    Rd = ControllerRollout(d)
    ms = Rd.sensor_state()
    Rd.set_sensor_state(np.zeros_like(ms))
    Rd.set_sensor_state(ms)
    R.advance(N, 3, TPU, H)
    Rd.advance(N, 3, TPU, H)
    assert_same(snap(g, R, N + 3), snap(d, Rd, N + 3), 'after the state round trip')
    # refusals: the setting, the state and the record stay
    s = snap(g, R, N + 3)
    for b, f, bad, msg in ((1, 0, 0, 'instance 1: mocap_ticks'), (2, 1, 4, 'instance 2: mocap_delay'), (3, 2, -1e-3, 'instance 3: sigma_p'),
                           (0, 13, np.nan, 'instance 0: lpf_x_joints'), (2, 15, 1.0, r'instance 2: reserved\[15\]')):
        sens = SENS.copy()
        sens[b, f] = bad
        with pytest.raises(RuntimeError, match=msg):
            R.set_sensors(sens, SEED)
    bad = R.sensor_state()
    bad[3, 0] = 2.5
    with pytest.raises(RuntimeError, match='instance 3: the sample count'):
        R.set_sensor_state(bad)
    assert_same(s, snap(g, R, N + 3), 'after the refused calls')
    same_bytes(R.sensors()[0], SENS, 'the setting after the refused calls')
    # set_state: the sensor state starts again from the state being set, the record from zero
    R.set_state(w.q, w.v)
    same_bytes(R.sensor_state(), sensors.state_init(g.L, w.q, w.v), 'sensor state after set_state')
    same_bytes(R.sensor_record(), np.zeros((B, 8)), 'record after set_state')
    same_bytes(R.measured()[0], w.q, 'measured after set_state')
    # set_sensors(None): the bytes of the rollout without the setting, and the getters refuse
    gb, Rb = w.fresh(tick_log=N, step_log=4)
    Rb.set_sensors(SENS, SEED)
    Rb.set_sensors(None)
    for call in (Rb.sensors, Rb.sensor_state, Rb.sensor_record, Rb.measured, lambda: Rb.set_sensor_state(ms), lambda: Rb.measure_dev(0, H, 1, 2, 3, 4)):
        with pytest.raises(RuntimeError, match='no sensors are set'):
            call()
    Rb.advance(0, N, TPU, H)
    assert_same(plain['end'], snap(gb, Rb, N, sens=False), 'after set_sensors(None) against never set')
    same_bytes(Rb.tick_log(), plain['tick_log'], 'tick log')
    same_bytes(gb.step_log(), plain['step_log'], 'step log')


def test_with_contact_feedback_latency_and_the_gait_step(world):
    """the world of test_gpu_mpc_latency.py's composition: ticks 20 .. 31 on contact_feedback_kit.raised_ground, an update every 3, gait_opt_freq 5 --
    updates 7 and 8 plain, 9 gradient (after tick 27), 10 line search (after tick 30): a gradient run comes before the first line search"""
    gw = ck.GroundWorld(world)
    k0, tpu, nt, freq = 20, 3, 12, 5
    lat = np.array([0.0, 0.012, 0.033, 0.0])
    ground = ck.raised_ground(gw, k0)
    runs = []
    for per_tick in (False, True):
        g, R = gw.fresh(k0, ground, feedback=1, tick_log=nt, step_log=4)
        gait = host.BatchGaitOptimizer(g)
        R.set_latency(lat)
        R.set_sensors(SENS, SEED)
        for a in (range(k0, k0 + nt) if per_tick else [k0]):
            R.advance(a, 1 if per_tick else nt, tpu, H, gait=gait, gait_opt_freq=freq)
        g.synchronize()
        assert not g.status()[1].any()
        s = snap(g, R, k0 + nt)
        s['cs'], s['feedback'], s['tick_log'], s['step_log'] = R.contact_state(), R.contact_feedback(), R.tick_log(), g.step_log()
        s['latency_record'], s['published'] = R.latency_record(), traj_bytes(R.published())
        s['contact_times'], s['counts'] = gait.contact_times()
        runs.append(s)
        gait.close()
    assert_same(runs[0], runs[1], 'one call per tick against one call')
    assert runs[0]['step_log'][:, 0, 58].astype(int).tolist() == [0, 0, 1, 2]          # plain, plain, gradient, line search
    assert runs[0]['sensor_record'][:, SR['ticks']].tolist() == [nt] * B
    assert runs[0]['sensor_record'][:, SR['samples']].tolist() == [12, 6, 4, 3]          # ticks 20 .. 31: every one, the even ones, 21 24 27 30, 20 25 30
