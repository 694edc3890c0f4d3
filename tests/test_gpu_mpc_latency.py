"""MPC computation latency in whole-controller rollouts (srbm_controller_set_latency, csrc/srbm_mpc_latency.hiph, through
ControllerRollout.set_latency / latency_record / published / publish_dev): with a latency set the control ticks read the PUBLISHED trajectories,
which follow the MPC's by base + per_iteration * (IPM iterations) seconds per instance, at the latest by one MPC period (the forced tick).

    1  a zero latency is no latency, byte for byte;
    2  the publish kernel alone, on both builds: due instances are copies, the others untouched, the forced call, the repeated call;
    3  the delay is real: until the first publication the ticks are those of a rollout that never updates;
    4  per-instance constants {0, 12, 27, 80 ms}: one call, one call per tick and the host-driven chain, bit for bit;
    5  the latency from the IPM iterations: the publication ticks are those srbm_latency_publish_ticks_host gives for the logged iteration counts;
    6  a rollout cut where instances are pending is the same rollout;
    7  on the raised ground with contact feedback and the gait step: one call against one call per tick;
    7b a rollout begun at a later tick with constant latencies only: one call, one call per tick and the chain, the record included;
    8  clone, set_state, refusals, set_latency(None).

The shapes of tests/controller_rollout_kit.py: 4 Config-B instances, ticks of 10 ms, an update every 5, 35 ticks or fewer.  The constant latencies keep
`due` at least 1 ms off every tick time (asserted from the inputs): fl(k h) + L against fl(j h) never sits on a rounding tie."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
from gpu_kit import same_bytes
from srbm_loader import host
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS as F, FLAG_UPDATE, publish_ticks
from test_gpu_controller_rollout import World, Dev, assert_same          # the batch of the rollout tests and its helpers

pytestmark = pytest.mark.gpu
B, H, TPU, NT = kit.B, kit.TICK_DT, kit.TPU, kit.NTICKS
CONST = np.array([0.0, 0.012, 0.027, 0.080])
MARGIN = 1e-3
ITERS = 11          # field of a step-log record: IPM iterations of the solve


@pytest.fixture(scope='module')
def world():
    return World()


def assert_margin(base, tpu, last_tick):
    """every due time of the constant latencies `base` is at least MARGIN off every tick time it is compared with"""
    for u in range(1, (last_tick - 1) // tpu + 1):
        t_start = np.float64(u * tpu) * H
        for lat in np.atleast_1d(base):
            due = t_start + lat
            assert min(abs(due - np.float64(j) * H) for j in range(u * tpu + 1, u * tpu + tpu + 1)) >= MARGIN, (u, lat)


def traj_bytes(arr):
    return np.frombuffer(bytes(arr), np.uint8)


def snap(g, R, next_tick, lat=True, q=None, v=None):
    """what a rollout leaves behind (test_gpu_controller_rollout.snapshot: the plant, the MPC's trajectories, q_des through the probe tick of a
    clone, which reads what the ticks read) and, with a latency set, the published trajectories and the latency record"""
    if q is None:
        q, v = R.state()
    probe = ControlTick(g.clone()).tick(q, v, next_tick * H)
    s = dict(q=q, v=v, trajectory=traj_bytes(g.get_trajectory()), q_des=probe['q_des'], probe_sol=probe['qp_sol'])
    if lat:
        s['published'], s['record'] = traj_bytes(R.published()), R.latency_record()
    return s


def record_after(e, t_pub, lat, overruns=0, n=1, max_lat=None, age=None):
    t_start = np.float64(e * TPU) * H
    return [e, n, overruns, t_pub, t_start, lat, lat if max_lat is None else max_lat, t_pub - t_start if age is None else age]


def test_a_zero_latency_is_no_latency(world):
    w, n = world, 12
    ga, Ra = w.fresh(tick_log=n, step_log=4)
    Ra.advance(0, n, TPU, H)
    gb, Rb = w.fresh(tick_log=n, step_log=4)
    Rb.set_latency(0)
    Rb.advance(0, n, TPU, H)
    assert_same(snap(ga, Ra, n, lat=False), snap(gb, Rb, n, lat=False), 'latency 0 against no latency')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    assert ga.step_log_count() == 2
    same_bytes(traj_bytes(Rb.published()), traj_bytes(gb.get_trajectory()), 'published against the MPC\'s at the end')
    rec = Rb.latency_record()
    want = record_after(2, 11 * H, 0.0, n=2, age=(6 * H - np.float64(5) * H) + (11 * H - np.float64(10) * H))
    same_bytes(rec, np.array([want] * B), 'latency record')
    with pytest.raises(RuntimeError, match='no latency is set'):
        Ra.latency_record()
    with pytest.raises(RuntimeError, match='no latency is set'):
        Ra.published()


@pytest.mark.parametrize('large', [False, True], ids=['standard', 'large'])
def test_the_publish_kernel_alone(world, large):
    w = world
    g = host.BatchMPC.cold_start(w.cfg, w.states, w.ees, large=large)
    R = ControllerRollout(g)
    lat = np.array([0.004, 0.030, 0.0, 0.030])          # at t = 0.07 with t_start = 0.05: instances 0 and 2 are due, 1 and 3 are not
    per = np.array([0.0, 0.0, 1e-4, 0.0])               # (instance 2: a few ms from its iterations, still due)
    R.set_latency(lat, per)
    old = [bytes(t) for t in g.get_trajectory()]
    same_bytes(traj_bytes(R.published()), traj_bytes(g.get_trajectory()), 'published at set_latency')
    rec0 = R.latency_record()
    same_bytes(rec0, np.array([[0, 0, 0, -1, 0, 0, 0, 0]] * B, float), 'record at set_latency')
    g.get_real_time_update(w.states, 5 * H, w.ees)           # the MPC's records move by one update
    iters = g.stats()[:, 4].astype(int)
    new = [bytes(t) for t in g.get_trajectory()]
    assert all(a != b for a, b in zip(old, new)) and np.all(iters > 0) and np.all(iters < 200)
    t_start, t = np.float64(5) * H, np.array([0.07, 0.07, 0.07, 0.07])
    p2 = per[2] * np.float64(iters[2])
    lat2 = lat[2] + p2
    assert t_start + lat[0] <= t[0] - MARGIN and t_start + lat2 <= t[2] - MARGIN and t_start + lat[1] >= t[1] + MARGIN
    dt = Dev(t)
    with pytest.raises(RuntimeError, match='update_number'):
        R.publish_dev(dt.p.value, -1, t_start, 0)
    with pytest.raises(RuntimeError, match='force'):
        R.publish_dev(dt.p.value, 1, t_start, 2)

    def state():
        g.synchronize()
        return [bytes(x) for x in R.published()], R.latency_record()
    R.publish_dev(dt.p.value, 1, t_start, 0)
    pub, rec = state()
    assert [pub[b] == new[b] for b in range(B)] == [True, False, True, False]
    assert [pub[b] == old[b] for b in range(B)] == [False, True, False, True]
    same_bytes(rec[[1, 3]], rec0[[1, 3]], 'records of the instances not due')
    age = t[0] - t_start
    same_bytes(rec[0], np.array([1, 1, 0, t[0], t_start, lat[0], lat[0], age]), 'record of instance 0')
    same_bytes(rec[2], np.array([1, 1, 0, t[2], t_start, lat2, lat2, age]), 'record of instance 2')
    assert [bytes(x) for x in g.get_trajectory()] == new          # the MPC's records are only read
    R.publish_dev(dt.p.value, 1, t_start, 0)                      # again: nothing is pending and due
    pub2, rec2 = state()
    assert pub2 == pub
    same_bytes(rec2, rec, 'records after the repeated call')
    R.publish_dev(dt.p.value, 1, t_start, 1)                      # forced: the rest, as overruns
    pub3, rec3 = state()
    assert pub3 == new
    same_bytes(rec3[[0, 2]], rec[[0, 2]], 'records of the instances published before')
    for b in (1, 3):
        same_bytes(rec3[b], np.array([1, 1, 1, t[b], t_start, lat[b], lat[b], age]), 'record of instance %d' % b)
    R.publish_dev(dt.p.value, 1, t_start, 1)                      # the same update number again, forced or not: nothing
    pub4, rec4 = state()
    assert pub4 == pub3
    same_bytes(rec4, rec3, 'records after the repeated forced call')


def test_the_delay_is_real(world):
    w, n, lat = world, 12, 0.027
    assert_margin([lat], TPU, n)
    ga, Ra = w.fresh(tick_log=n, step_log=4)
    Ra.set_latency(lat)
    pubs = []
    for k in range(n):                                   # (one call per tick is one call: test 4)
        Ra.advance(k, 1, TPU, H)
        pubs.append(Ra.latency_record()[:, 1].copy())
    gb, Rb = w.fresh(tick_log=n, step_log=4)
    Rb.advance(0, n, 50, H)                              # never updates
    assert gb.step_log_count() == 0 and ga.step_log_count() == 2
    iters = ga.step_log()[:, :, ITERS].T.astype(np.int32)          # [B][2]
    want_tick, want_over = publish_ticks(ga.L, 0, n, TPU, H, lat, 0.0, iters)
    assert np.array_equal(want_tick, [[8, -1]] * B) and not want_over.any()
    got_tick = np.array([[min(k for k in range(n) if pubs[k][b] >= u) if pubs[-1][b] >= u else -1 for u in (1, 2)] for b in range(B)])
    assert np.array_equal(got_tick, want_tick), (got_tick, want_tick)
    la, lb = Ra.tick_log().copy(), Rb.tick_log().copy()
    assert [k for k in range(n) if int(la[k, 0, F['flags']]) & FLAG_UPDATE] == [5, 10] and not (lb[:, :, F['flags']].astype(int) & FLAG_UPDATE).any()
    la[:, :, F['flags']] = la[:, :, F['flags']].astype(int) & ~FLAG_UPDATE
    first = 8
    same_bytes(la[:first], lb[:first], 'the ticks before the first publication against the rollout that never updates')
    for b in range(B):
        assert la[first, b].tobytes() != lb[first, b].tobytes(), b
    same_bytes(Ra.latency_record(), np.array([record_after(1, 8 * H, lat)] * B), 'latency record')


def run_chain(g, R, q, v, first, ticks, tpu, first_update=0):
    """the loop driven from the host: srbm_controller_publish_dev, srbm_control_tick_dev, srbm_wb_plant_step_dev, srbm_get_real_time_update_dev; after
    every publication the published record of the instance is held to the MPC record read back after that update.  -> the final (q, v)"""
    T = ControlTick(g)
    n = g.batch
    d = dict(q=Dev(q), v=Dev(v), t=Dev(np.zeros(n)), control=Dev(np.zeros((n, 36))), qp_sol=Dev(np.zeros((n, 30))), status=Dev(np.zeros((n, 2), np.int32)),
             contact=Dev(np.zeros((n, 4), np.int32)), state=Dev(np.zeros((n, 13))), ee=Dev(np.zeros((n, 4, 3))))
    mpc_after, in_force, published = {first_update: [bytes(t) for t in g.get_trajectory()]}, np.zeros(n), 0          # (begun later: the found ones go as first_update)
    for k in range(first, first + ticks):
        g.synchronize()
        d['t'].put(np.full(n, k * H))
        e = (k - 1) // tpu if k >= 1 else 0
        if e >= 1:
            R.publish_dev(d['t'].p.value, e, np.float64(e * tpu) * H, int(k % tpu == 0))
            g.synchronize()
            now = R.latency_record()[:, 0]
            pubs = R.published()
            for b in np.nonzero(now != in_force)[0]:
                assert now[b] == e and bytes(pubs[b]) == mpc_after[e][b], (k, b)
                published += 1
            in_force = now
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        R.plant_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['qp_sol'].p.value, d['status'].p.value)
        if k > 0 and k % tpu == 0:
            g.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
            g.synchronize()
            mpc_after[k // tpu] = [bytes(t) for t in g.get_trajectory()]
    g.synchronize()
    return d['q'].get(), d['v'].get(), published


def test_per_instance_constants_three_ways(world):
    w = world
    assert_margin(CONST, TPU, NT)
    ga, Ra = w.fresh(tick_log=NT, step_log=8)
    Ra.set_latency(CONST)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = w.fresh(tick_log=NT, step_log=8)
    Rb.set_latency(CONST)
    for k in range(NT):
        Rb.advance(k, 1, TPU, H)
    gc, Rc = w.fresh(step_log=8)
    Rc.set_latency(CONST)
    qc, vc, published = run_chain(gc, Rc, w.q, w.v, 0, NT, TPU)
    sa = snap(ga, Ra, NT)
    assert_same(sa, snap(gb, Rb, NT), 'one call per tick against one call')
    assert_same(sa, snap(gc, Rc, NT, q=qc, v=vc), 'the host-driven chain against one call')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log: one call per tick')
    same_bytes(ga.step_log(), gb.step_log(), 'step log: one call per tick')
    same_bytes(ga.step_log(), gc.step_log(), 'step log: the chain')
    # 35 ticks: updates 1 .. 6 after ticks 5 .. 30; published before k + 1, k + 2, k + 3 and the forced k + 5 (update 6 of the last: beyond the end)
    rec = sa['record']
    assert published == 6 * 3 + 5
    assert rec[:, 0].tolist() == [6, 6, 6, 5] and rec[:, 1].tolist() == [6, 6, 6, 5] and rec[:, 2].tolist() == [0, 0, 0, 5]
    assert rec[:, 3].tolist() == [31 * H, 32 * H, 33 * H, 30 * H] and rec[:, 4].tolist() == [30 * H, 30 * H, 30 * H, 25 * H]
    same_bytes(rec[:, 5], CONST, 'L of the last publication')
    same_bytes(rec[:, 6], CONST, 'max L')
    want_tick, want_over = publish_ticks(ga.L, 0, NT, TPU, H, CONST, 0.0, np.zeros((B, 6), np.int32))
    k = TPU * np.arange(1, 7)
    assert np.array_equal(want_tick, [k + 1, k + 2, k + 3, np.where(k + 5 < NT, k + 5, -1)]) and want_over.sum(axis=1).tolist() == [0, 0, 0, 5]
    # the latencies did something: another rollout than without them, and instance 0 (L = 0) is the rollout without them
    gd, Rd = w.fresh(tick_log=NT)
    Rd.advance(0, NT, TPU, H)
    la, ld = Ra.tick_log(), Rd.tick_log()
    same_bytes(la[:, 0], ld[:, 0], 'tick log of the instance with L = 0 against no latency')
    for b in (1, 2, 3):
        assert la[:, b].tobytes() != ld[:, b].tobytes(), b


@pytest.mark.parametrize('k0', [13, 18])
@pytest.mark.parametrize('lat', [np.zeros(4), CONST], ids=['zero', 'constants'])
def test_begun_at_a_later_tick_three_ways(world, lat, k0):
    """a rollout BEGUN at tick k0 > ticks_per_update on a state just set, constant latencies only: update 0 is in force and e = (k0 - 1) / 5 >= 2, so
    whatever the rule would have published before k0 is due before the first tick -- ticks on which the host's skip rule, made for a rollout that has
    run since the update started, launches for nobody.  The entry in one call, in one call per tick and the chain that launches the kernel before
    every tick leave the same bytes, the latency record included"""
    w, n = world, 12
    assert_margin(lat, TPU, k0 + n)
    ga, Ra = w.fresh(tick_log=n, step_log=4)
    Ra.set_latency(lat)
    Ra.advance(k0, 1, TPU, H)
    e, t_start = (k0 - 1) // TPU, np.float64(((k0 - 1) // TPU) * TPU) * H
    due = np.array([t_start + x <= k0 * H for x in lat])
    assert due.sum() >= 3 and not Ra.latency_record()[~due, 1].any()
    for b in np.nonzero(due)[0]:          # published before the first tick: the trajectories found, as update e
        same_bytes(Ra.latency_record()[b], np.array([e, 1, 0, k0 * H, t_start, lat[b], lat[b], k0 * H - t_start]), 'record of instance %d after the first tick' % b)
    Ra.advance(k0 + 1, n - 1, TPU, H)
    gb, Rb = w.fresh(tick_log=n, step_log=4)
    Rb.set_latency(lat)
    Rb.advance(k0, n, TPU, H)
    gc, Rc = w.fresh(step_log=4)
    Rc.set_latency(lat)
    qc, vc, _ = run_chain(gc, Rc, w.q, w.v, k0, n, TPU, first_update=e)
    gd, Rd = w.fresh(tick_log=n, step_log=4)
    Rd.set_latency(lat)
    for k in range(k0, k0 + n):
        Rd.advance(k, 1, TPU, H)
    sb = snap(gb, Rb, k0 + n)
    assert_same(sb, snap(ga, Ra, k0 + n), 'one tick and the rest against one call')
    assert_same(sb, snap(gd, Rd, k0 + n), 'one call per tick against one call')
    assert_same(sb, snap(gc, Rc, k0 + n, q=qc, v=vc), 'the host-driven chain against one call')
    same_bytes(Rb.tick_log(), Rd.tick_log(), 'tick log: one call per tick')
    same_bytes(gb.step_log(), gd.step_log(), 'step log: one call per tick')
    same_bytes(gb.step_log(), gc.step_log(), 'step log: the chain')
    assert sb['record'][:, 0].min() >= e


def test_latency_from_the_iterations(world):
    w = world
    base, per = 0.0004, np.array([0.0007, 0.0011, 0.0015, 0.0019])
    ga, Ra = w.fresh(tick_log=NT, step_log=8)
    Ra.set_latency(base, per)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = w.fresh(tick_log=NT, step_log=8)
    Rb.set_latency(base, per)
    ticks = np.full((B, 6), -1)
    seen = np.zeros(B)
    for k in range(NT):
        Rb.advance(k, 1, TPU, H)
        now = Rb.latency_record()[:, 0]
        for b in np.nonzero(now != seen)[0]:
            ticks[b, int(now[b]) - 1] = k
        seen = now
    assert_same(snap(ga, Ra, NT), snap(gb, Rb, NT), 'one call per tick against one call')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    iters = ga.step_log()[:, :, ITERS].T.astype(np.int32)
    want_tick, want_over = publish_ticks(ga.L, 0, NT, TPU, H, base, per, iters)
    print('IPM iterations per instance and update:', iters.tolist(), 'publication ticks:', want_tick.tolist())
    assert np.array_equal(ticks, want_tick), (ticks, want_tick)
    assert any(len(set(want_tick[:, u])) > 1 for u in range(6))          # the four instances do not all publish on the same tick
    rec = Ra.latency_record()
    assert np.array_equal(rec[:, 2], want_over.sum(axis=1)) and np.array_equal(rec[:, 1], (want_tick >= 0).sum(axis=1))
    last = [max(u for u in range(6) if want_tick[b, u] >= 0) for b in range(B)]
    p = per * iters[np.arange(B), last]
    same_bytes(rec[:, 5], base + p, 'L of the last publication from its iteration count')


def test_cut_anywhere(world):
    w = world
    ga, Ra = w.fresh(tick_log=NT, step_log=8)
    Ra.set_latency(CONST)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = w.fresh(tick_log=NT, step_log=8)
    Rb.set_latency(CONST)
    cuts = [0, 6, 7, 9, 17, 23, NT]          # after the update of tick 5: three instances pending before tick 6, two before 7, one before 9; 17, 23 likewise
    for a, b in zip(cuts[:-1], cuts[1:]):
        Rb.advance(a, b - a, TPU, H)
        if b < NT:
            assert (Rb.latency_record()[:, 0] < (b - 1) // TPU).any(), b          # somebody is pending at the cut
    assert_same(snap(ga, Ra, NT), snap(gb, Rb, NT), 'the cut rollout against one call')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')


def test_with_contact_feedback_and_the_gait_step(world):
    """the world of test_gpu_gait_controller_rollout.py on contact_feedback_kit.raised_ground: ticks 20 .. 31, an update every 3, gait_opt_freq 5 --
    updates 7 and 8 plain, 9 gradient (after tick 27), 10 line search (after tick 30).  (The first update of a rollout must not be a line search:
    nothing has read the contact times yet.)  Instance 2's 33 ms exceed the period of 30 ms: every publication of it is forced"""
    w = world
    gw = ck.GroundWorld(w)
    k0, tpu, nt, freq = 20, 3, 12, 5
    lat, per = np.array([0.0, 0.012, 0.033, 0.0004]), np.array([0.0, 0.0, 0.0, 0.0007])
    assert_margin(lat[:3], tpu, k0 + nt)
    ground = ck.raised_ground(gw, k0)
    runs = []
    for per_tick in (False, True):
        g, R = gw.fresh(k0, ground, feedback=1, tick_log=nt, step_log=4)
        gait = host.BatchGaitOptimizer(g)
        R.set_latency(lat, per)
        for a in (range(k0, k0 + nt) if per_tick else [k0]):
            R.advance(a, 1 if per_tick else nt, tpu, H, gait=gait, gait_opt_freq=freq)
        g.synchronize()
        assert not g.status()[1].any()
        s = snap(g, R, k0 + nt)
        s['cs'], s['feedback'], s['tick_log'], s['step_log'] = R.contact_state(), R.contact_feedback(), R.tick_log(), g.step_log()
        s['contact_times'], s['counts'] = gait.contact_times()
        runs.append(s)
        gait.close()
    assert_same(runs[0], runs[1], 'one call per tick against one call')
    assert runs[0]['step_log'][:, 0, 58].astype(int).tolist() == [0, 0, 1, 2]          # plain, plain, gradient, line search
    assert runs[0]['feedback'][:, :, 0].sum() > 0                                         # contact feedback moved a touch-down
    rec = runs[0]['record']
    # before tick 31 update 10 is in force where L = 0; instance 2 was forced before ticks 21, 24, 27 and 30
    assert rec[0, 0] == 10 and rec[0, 2] == 0 and rec[2, 0] == 9 and rec[2, 2] == rec[2, 1] == 4, rec[:, :3]


def test_clone_reset_refusals(world):
    w = world
    assert_margin(CONST, TPU, 18)
    g, R = w.fresh(tick_log=18, step_log=4)
    R.set_latency(CONST)
    R.advance(0, 8, TPU, H)
    assert R.latency_record()[:, 0].tolist() == [1, 1, 0, 0]          # the clone is made while instances 2 and 3 are pending
    c = g.clone()
    Rc = ControllerRollout(c)
    assert_same(snap(g, R, 8), snap(c, Rc, 8), 'the clone')
    R.advance(8, 10, TPU, H)
    Rc.advance(8, 10, TPU, H)
    s = snap(g, R, 18)
    assert_same(s, snap(c, Rc, 18), 'the clone, 10 ticks on')
    assert s['record'][:, 0].tolist() == [3, 3, 2, 2] and s['published'].tobytes() != s['trajectory'].tobytes()
    # refusals: plant, trajectories, published set, record, q_des and the log cursors stay
    cur = (R.tick_log_count(), g.step_log_count())
    for args, msg in ((([0.0, -0.001, 0.0, 0.0],), 'instance 1: base'), ((0.0, [0.0, 0.0, np.nan, 0.0]), 'instance 2: per_iteration'),
                      (([0.0, 0.0, 0.0, np.inf],), 'instance 3: base')):
        with pytest.raises(RuntimeError, match=msg):
            R.set_latency(*args)
        assert_same(s, snap(g, R, 18), 'after the refused set_latency %s' % (args,))
    horizon = w.cfg['num_nodes'] * w.cfg['integrator_dt']
    assert 2 * 50 * H >= horizon > 50 * H
    with pytest.raises(RuntimeError, match=r'twice the MPC period.* is 1\b.*1\.0'):
        R.advance(18, 2, 50, H)                          # accepted without a latency (test_gpu_controller_rollout.py), refused with one
    assert_same(s, snap(g, R, 18), 'after the refused advance')
    assert (R.tick_log_count(), g.step_log_count()) == cur
    # set_state: what is in force is what the MPC holds, the record starts again
    R.set_state(w.q, w.v)
    same_bytes(traj_bytes(R.published()), traj_bytes(g.get_trajectory()), 'published after set_state')
    same_bytes(R.latency_record(), np.array([[0, 0, 0, -1, 0, 0, 0, 0]] * B, float), 'record after set_state')
    # set_latency(None): today's bytes
    ga, Ra = w.fresh(tick_log=12, step_log=4)
    Ra.advance(0, 12, TPU, H)
    gb, Rb = w.fresh(tick_log=12, step_log=4)
    Rb.set_latency(0.027)
    Rb.set_latency(None)
    with pytest.raises(RuntimeError, match='no latency is set'):
        Rb.latency_record()
    Rb.advance(0, 12, TPU, H)
    assert_same(snap(ga, Ra, 12, lat=False), snap(gb, Rb, 12, lat=False), 'after set_latency(None) against never set')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
