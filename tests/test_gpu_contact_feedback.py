"""Contact feedback from the ground in whole-controller rollouts (srbm_controller_set_contact_feedback, srbm_controller_get_contact_feedback,
srbm_controller_contact_feedback_dev; csrc/srbm_contact_feedback.hiph through bilevel-gait-gen_amd/controller_rollout.py):

    1  the kernel alone: bitwise the existing srbm_adjust_for_current_contacts, bit-exact the oracle's AdjustForCurrentContacts, the feedback
       record counts exactly the moved feet; the touch-down-index error; both builds;
    2  one update tick against the host-driven chain of the four device entries, against the same call with feedback off;
    3  a rollout on a raised ground three ways, with a moved touch-down and a flagged foot refused for being 70 ms or more away inside;
    4  off means absent, and on without a ground (or under kind 0) is refused with the batch untouched.

The world of 2..4 is test_gpu_controller_rollout.py's (4 Config-B instances after one cold start, ticks of 10 ms) with the torque-driven plant on a
ground; the rollouts begin at tick 20 (t = 0.2), so that the first planned touch-down (t = 0.3) comes within 70 ms inside them."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
from contact_feedback_kit import GroundWorld, classify, flat_ground, knot_times, posxy, raised_ground, traj_bytes, LO, TD, GUARD
from gpu_kit import same_bytes
from oracle_py import OracleMPC
from srbm_loader import host
from srbm_loader.controller_rollout import ControllerRollout, decode_ground_word, PLANT_QP_ACCELERATION
from srbm_loader.workloads import config_b_instance, instances
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same           # the kind-0 tests' batch and helpers

pytestmark = pytest.mark.gpu
B, H = kit.B, kit.TICK_DT
ERR_TD_INDEX = 64
K0, NT, TPU = 20, 12, 3         # the rollouts: ticks 20 .. 31, updates after ticks 21, 24, 27, 30


def feedback_chain(*args, **kw):
    return ck.feedback_chain(Dev, *args, **kw)


def ground_snapshot(w, g, R, next_tick):
    return ck.ground_snapshot(snapshot, w, g, R, next_tick)


# ---- 1. the kernel alone ----
class KernelCase:
    """4 Config-B instances after the cold start and two host-driven steps, on the oracle (one OracleMPC per instance, computed once and cloned by
    the tests) with the inputs of every solve recorded, so that a device batch of either build replays them"""

    def __init__(self):
        self.cfg = host.load_config('a1_configuration')
        self.states, self.ees = instances(self.cfg, config_b_instance, B)
        self.ees = np.asarray(self.ees, float).reshape(B, 4, 3)
        self.oracles, self.steps = [], []
        for b in range(B):
            o = OracleMPC(self.cfg)
            o.set_warmstart(self.states[b]); o.initial_run(self.states[b], self.ees[b])
            self.oracles.append(o)
        dt = self.cfg['integrator_dt']
        for i in range(2):
            t = i * dt
            st = np.array([o.states()[1] for o in self.oracles])
            ee = np.array([[[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)] for o in self.oracles])
            for b, o in enumerate(self.oracles):
                o.rti(st[b], t, ee[b])
            self.steps.append((st, t, ee))

    def device(self, large, steps=True):
        g = host.BatchMPC.cold_start(self.cfg, self.states, self.ees, large=large)
        for st, t, ee in (self.steps if steps else []):
            g.get_real_time_update(st, t, ee)
        return g


@pytest.fixture(scope='module')
def kernel_case():
    return KernelCase()


def feedback_on_arrays(g, t, cs):
    """srbm_controller_contact_feedback_dev on a batch that has a plant state (which allocates the feedback record) -> fb"""
    R = ControllerRollout(g)
    R.set_state(np.zeros(19), np.zeros(18))
    dt_, dc = Dev(t), Dev(cs)
    R.contact_feedback_dev(dt_.p.value, dc.p.value)
    g.synchronize()
    return R.contact_feedback()


@pytest.mark.parametrize('large', [False, True], ids=['standard', 'large'])
def test_the_kernel_alone_against_the_existing_entry_and_the_oracle(kernel_case, large):
    """per instance the four feet in four cases, chosen from its own knot tables: A flagged 50 .. 53 ms before its touch-down (moved), B flagged
    80 .. 83 ms before its own (its touch-down is first set 30 ms later: not moved), C flagged while the plan holds it, D not flagged.  Margins
    asserted on the host: A's distance in [45, 65] ms, B's at least 75 ms, A's new knot within 95 ms of the old one (the guard is 100 ms)"""
    kc = kernel_case
    g = kc.device(large)
    oracles = [o.clone() for o in kc.oracles]
    for b, o in enumerate(oracles):                  # the batch replayed the oracle's steps: the same knot tables, bit for bit
        kn = g.knots(b)
        for e in range(4):
            ko = o.knots(e)
            assert kn['nk'][e] == ko['K'] and np.array_equal(kn['times'][e, :ko['K']], ko['times']), (b, e)
    t_ref = 2 * kc.cfg['integrator_dt']
    arr = np.zeros((B, 4, 8))
    roles, new_ct = [], []
    for b in range(B):
        kn = g.knots(b)
        swing = [e for e in range(4) if classify(kn, e, t_ref)[0] != 'held']
        held = [e for e in range(4) if e not in swing]
        assert len(swing) == 2 and len(held) == 2, (b, swing)
        ct = [posxy(kn, e)[0].copy() for e in range(4)]
        a, bf = swing
        ia = min(i for i in range(len(ct[a])) if ct[a][i] > t_ref)
        ib = min(i for i in range(len(ct[bf])) if ct[bf][i] > t_ref)
        assert posxy(kn, a)[1][ia] == TD and posxy(kn, bf)[1][ib] == TD and ct[a][ia] == ct[bf][ib], b
        ct[bf][ib] += 0.03
        assert ct[bf][ib] < ct[bf][ib + 1] - 0.1, b
        for e in range(4):
            assert len(ct[e]) <= 8
            arr[b, e, :len(ct[e])] = ct[e]
        roles.append(dict(A=a, B=bf, C=held[0], D=held[1], td=ct[a][ia]))
        new_ct.append(ct)
    g.update_contact_times(arr)
    for b, o in enumerate(oracles):
        o.set_contact_times(new_ct[b])
    t = np.array([roles[b]['td'] - (0.05 + 0.001 * b) for b in range(B)])
    flags = np.zeros((B, 4), np.int32)
    cs = np.zeros((B, 4, 3))
    for b, r in enumerate(roles):
        kn = g.knots(b)
        ko = [oracles[b].knots(e) for e in range(4)]
        for e in range(4):
            assert np.array_equal(kn['times'][e, :ko[e]['K']], ko[e]['times']), (b, e)
        what = {k: classify(kn, r[k], t[b]) for k in 'ABCD'}
        assert what['A'][0] == 'moved' and 0.045 <= what['A'][1] <= 0.065, (b, what)
        assert what['B'][0] == 'far' and what['B'][1] >= 0.075, (b, what)
        assert what['C'][0] == 'held' and what['D'][0] == 'held', (b, what)
        times, kinds, _ = posxy(kn, r['A'])
        up = min(i for i in range(len(times)) if t[b] < times[i])
        assert kinds[up] == TD and abs(times[up] - t[b]) <= GUARD - 0.005, b
        for k in 'ABC':
            flags[b, r[k]] = 1
            cs[b, r[k]] = [1.0, 0.1 * r[k] + 0.01, -0.2 + 0.03 * b]          # in contact, with anchors that are not zero
        cs[b, r['D']] = [0.0, 0.4, -0.4]
    before = [knot_times(g, b) for b in range(B)]
    ga, gb = g.clone(), g.clone()
    fb = feedback_on_arrays(ga, t, cs)
    gb.adjust_for_current_contacts(t, flags)
    # (i) the same bytes as the existing entry with the int flags
    same_bytes(traj_bytes(ga), traj_bytes(gb), 'trajectory records: the feedback kernel against srbm_adjust_for_current_contacts')
    for x, y in zip(ga.status(), gb.status()):
        assert np.array_equal(x, y)
    assert not ga.status()[1].any()
    # (ii) the oracle, with the comparison of the a17 test of test_gpu_parity.py
    for b, o in enumerate(oracles):
        o.adjust_for_current_contacts(t[b], flags[b])
        kn = ga.knots(b)
        for e in range(4):
            ko = o.knots(e)
            assert kn['nk'][e] == ko['K'] and np.array_equal(kn['times'][e, :ko['K']], ko['times']), (b, e)
    # (iii) the record counts exactly the moved feet; and only A's knots moved
    want = np.zeros((B, 4, 2)); want[:, :, 1] = -1.0
    for b, r in enumerate(roles):
        want[b, r['A']] = [1.0, t[b]]
        after = knot_times(ga, b)
        for e in range(4):
            assert np.array_equal(after[e], before[b][e]) == (e != r['A']), (b, e)
    same_bytes(fb, want, 'the feedback record')
    # a second run at the same time finds A held by the plan: nothing moves, nothing is counted
    R = ControllerRollout(ga)
    dt_, dc = Dev(t), Dev(cs)
    R.contact_feedback_dev(dt_.p.value, dc.p.value)
    ga.synchronize()
    same_bytes(R.contact_feedback(), want, 'the feedback record after a second run')
    same_bytes(traj_bytes(ga), traj_bytes(gb), 'trajectory records after a second run')
    R.set_state(np.zeros(19), np.zeros(18))          # ... and set_state resets the record
    assert np.array_equal(R.contact_feedback()[:, :, 0], np.zeros((B, 4))) and np.all(R.contact_feedback()[:, :, 1] == -1.0)
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_state'):
        ControllerRollout(g.clone()).contact_feedback_dev(dt_.p.value, dc.p.value)


@pytest.mark.parametrize('large', [False, True], ids=['standard', 'large'])
def test_the_touch_down_index_error_is_the_existing_entrys(kernel_case, large):
    """right after the cold start a foot whose table begins with its lift-off gets a swing of 50 ms; 10 ms BEFORE that first knot the next
    touch-down is 60 ms away but the knot above that time is the lift-off itself, not a touch-down: the reference throws (on the time already),
    both entries raise bit 64 on the same instances and leave the same bytes, and nothing is counted for that foot"""
    g = kernel_case.device(large, steps=False)
    arr = np.zeros((B, 4, 8))
    t = np.zeros(B)
    foot = []
    for b in range(B):
        kn = g.knots(b)
        first_lo = [e for e in range(4) if kn['kinds'][e, 0] == LO]
        assert first_lo, b
        e0 = first_lo[0]
        for e in range(4):
            ct = posxy(kn, e)[0].copy()
            if e == e0:
                assert posxy(kn, e)[1][1] == TD
                ct[1] = ct[0] + 0.05
            arr[b, e, :len(ct)] = ct
        t[b] = kn['times'][e0, 0] - 0.01
        foot.append(e0)
    g.update_contact_times(arr)
    cs = np.zeros((B, 4, 3)); flags = np.zeros((B, 4), np.int32)
    for b, e0 in enumerate(foot):
        cs[b, e0] = [1.0, 0.2, -0.1]; flags[b, e0] = 1
    ga, gb = g.clone(), g.clone()
    fb = feedback_on_arrays(ga, t, cs)
    gb.adjust_for_current_contacts(t, flags)
    same_bytes(traj_bytes(ga), traj_bytes(gb), 'trajectory records')
    ea, eb = ga.status()[1], gb.status()[1]
    assert np.array_equal(ea, eb) and np.all(ea & ERR_TD_INDEX), (ea, eb)
    same_bytes(traj_bytes(ga), traj_bytes(g), 'the refused foot leaves the tables as they were')
    assert np.all(fb[:, :, 0] == 0) and np.all(fb[:, :, 1] == -1.0)


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def gw(world):
    return GroundWorld(world)


# ---- 2. one update tick ----
def test_one_update_tick_against_the_host_driven_chain_and_against_feedback_off(world, gw):
    """tick 24 (t = 0.24, an update tick at 3 ticks per update) from a state set for it, with one swing foot per instance flagged 60 ms before its
    planned touch-down at 0.3"""
    w, k = world, 24
    t = k * H
    ground = flat_ground(gw, k)
    q, v, _ = gw.start(k)
    plan, feet = gw.plan(t), gw.feet(q)
    cs = np.zeros((B, 4, 3))
    flagged = []
    for b in range(B):
        kn = w.base.knots(b)
        e = [e for e in range(4) if not plan[b, e]][b % 2]
        what, away = classify(kn, e, t)
        assert what == 'moved' and 0.045 <= away <= 0.065, (b, e, what, away)          # 70 ms - 5 ms at least
        cs[b, e] = [1.0, feet[b, e, 0], feet[b, e, 1]]
        flagged.append(e)
    res = {}
    for name, fbk in (('on', 1), ('off', 0)):
        g, R = gw.fresh(k, ground, feedback=fbk, tick_log=1, step_log=1)
        R.set_contact_state(cs)
        R.advance(k, 1, TPU, H)
        res[name] = dict(g=g, R=R, snap=ground_snapshot(w, g, R, k + 1), tick=R.tick_log(), step=g.step_log(), fb=R.contact_feedback())
        assert g.step_log_count() == 1 and not g.status()[1].any()
    gc, Rc = gw.fresh(k, ground, step_log=1)
    fb_chain = feedback_chain(gc, Rc, q, v, cs, k, 1, TPU)
    assert_same(res['on']['snap'], ground_snapshot(w, gc, Rc, k + 1), 'feedback on against the host-driven chain')
    same_bytes(res['on']['step'], gc.step_log(), 'step log against the chain')
    same_bytes(res['on']['fb'], fb_chain, 'feedback record against the chain')
    want = np.zeros((B, 4, 2)); want[:, :, 1] = -1.0
    for b, e in enumerate(flagged):
        want[b, e] = [1.0, t]
    same_bytes(res['on']['fb'], want, 'feedback record')
    assert np.all(res['off']['fb'][:, :, 0] == 0)
    # the tick ran before the snap: its record is the same bytes; the schedule the update started from is not
    same_bytes(res['on']['tick'], res['off']['tick'], 'the tick record with feedback on and off')
    assert not np.array_equal(res['on']['snap']['trajectory'], res['off']['snap']['trajectory'])
    for b, e in enumerate(flagged):
        on, off = knot_times(res['on']['g'], b), knot_times(res['off']['g'], b)
        assert on[e].tolist() != off[e].tolist() and t in on[e] and t not in off[e], (b, e, on[e], off[e])
        for f in range(4):
            if f != e:
                assert len(on[f]) == len(off[f]) and np.array_equal(on[f], off[f]), (b, f)


# ---- 3. a rollout on a raised ground ----
def test_a_rollout_on_a_raised_ground_three_ways_with_a_moved_and_a_refused_touch_down_inside(world, gw):
    w = world
    ground = raised_ground(gw, K0)
    q, v, _ = gw.start(K0)
    ga, Ra = gw.fresh(K0, ground, feedback=1, tick_log=NT, step_log=4)
    Ra.advance(K0, NT, TPU, H)
    # one call per tick; before every update tick the host derives what the feedback must do, from field 63 of the record of tick k - 1 (the
    # ground's flags at t_k) and the knot tables read back
    gb, Rb = gw.fresh(K0, ground, feedback=1, tick_log=NT, step_log=4)
    moved = far = held = 0
    want = np.zeros((B, 4, 2)); want[:, :, 1] = -1.0
    for k in range(K0, K0 + NT):
        if k % TPU == 0 and k > K0:
            word = decode_ground_word(Rb.tick_log(k - 1 - K0, 1)[0, :, 63])
            assert np.array_equal(word['in_contact'], Rb.contact_state()[:, :, 0] == 1)
            for b in range(B):
                kn = gb.knots(b)
                for e in range(4):
                    if word['in_contact'][b, e]:
                        what, away = classify(kn, e, k * H)
                        assert what != 'error', (k, b, e)
                        moved += what == 'moved'; far += what == 'far'; held += what == 'held'
                        if what == 'moved':
                            want[b, e] = [want[b, e, 0] + 1.0, k * H]
        Rb.advance(k, 1, TPU, H)
        if k % TPU == 0:
            same_bytes(Rb.contact_feedback(), want, 'feedback record after tick %d' % k)
    print('flagged feet at the update ticks: %d moved, %d refused 70 ms or more away, %d held by the plan' % (moved, far, held))
    assert moved >= 1 and far >= 1, (moved, far, held)
    gc, Rc = gw.fresh(K0, ground, step_log=4)
    fb_chain = feedback_chain(gc, Rc, q, v, np.zeros((B, 4, 3)), K0, NT, TPU)
    sa = ground_snapshot(w, ga, Ra, K0 + NT)
    for name, g, R in (('one call per tick', gb, Rb), ('host-driven chain', gc, Rc)):
        assert_same(sa, ground_snapshot(w, g, R, K0 + NT), name)
    same_bytes(Ra.contact_feedback(), want, 'feedback record: one call')
    same_bytes(fb_chain, want, 'feedback record: the chain')
    assert Ra.tick_log_count() == Rb.tick_log_count() == NT and Rc.tick_log_count() == 0
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log: one call against one per tick')
    assert ga.step_log_count() == gb.step_log_count() == gc.step_log_count() == 4
    same_bytes(ga.step_log(), gb.step_log(), 'step log: one call against one per tick')
    same_bytes(ga.step_log(), gc.step_log(), 'step log: one call against the chain')
    assert not ga.status_accumulated()[:, 0].any()
    # ... and the feedback matters: the same rollout with it off ends on other trajectories
    gd, Rd = gw.fresh(K0, ground, feedback=0)
    Rd.advance(K0, NT, TPU, H)
    assert not np.array_equal(traj_bytes(gd), sa['trajectory'])


# ---- 4. off means absent ----
def test_feedback_off_is_absent_and_on_without_a_ground_is_refused(world, gw):
    w, n = world, 8
    ground = raised_ground(gw, K0)

    def run(prepare):
        g, R = gw.fresh(K0, ground, tick_log=n, step_log=4)
        g, R = prepare(g, R)
        R.advance(K0, n, TPU, H)
        return ground_snapshot(w, g, R, K0 + n), R.tick_log(), g.step_log(), R.contact_feedback()

    def set_off(g, R):
        R.set_contact_feedback(0)
        return g, R

    def on_and_off(g, R):
        R.set_contact_feedback(1); R.set_contact_feedback(0)
        return g, R

    def cloned(g, R):
        R.set_contact_feedback(1); R.set_contact_feedback(0)
        c = g.clone()
        Rc = ControllerRollout(c)
        Rc.tick_log_enable(n); c.step_log_enable(4)
        return c, Rc
    never = run(lambda g, R: (g, R))
    for name, prepare in (('set to 0', set_off), ('on and off again', on_and_off), ('a clone of such a batch', cloned)):
        got = run(prepare)
        assert_same(never[0], got[0], name)
        for i, what in ((1, 'tick log'), (2, 'step log'), (3, 'feedback record')):
            same_bytes(never[i], got[i], '%s: %s' % (name, what))
    assert np.all(never[3][:, :, 0] == 0) and np.all(never[3][:, :, 1] == -1.0)
    # a clone carries the setting: it ends where the original ends, and elsewhere than with it off
    g, R = gw.fresh(K0, ground, feedback=1)
    c = g.clone()
    Rc = ControllerRollout(c)
    R.advance(K0, n, TPU, H); Rc.advance(K0, n, TPU, H)
    assert_same(ground_snapshot(w, g, R, K0 + n), ground_snapshot(w, c, Rc, K0 + n), 'a clone of a batch with feedback on')
    same_bytes(R.contact_feedback(), Rc.contact_feedback(), 'its feedback record')
    assert R.contact_feedback()[:, :, 0].sum() >= 1
    # on without a ground, and on under kind 0 with a ground: refused, naming the setting, with the batch untouched
    for name, kw in (('kind 1 without a ground', dict(ground=None)), ('kind 0 with a ground', dict(ground=ground, kind=PLANT_QP_ACCELERATION))):
        g, R = gw.fresh(K0, feedback=1, tick_log=2, step_log=1, **kw)
        s0 = ground_snapshot(w, g, R, K0)
        with pytest.raises(RuntimeError, match='srbm_controller_set_contact_feedback'):
            R.advance(K0, 2, TPU, H)
        assert (R.tick_log_count(), g.step_log_count()) == (0, 0), name
        assert_same(s0, ground_snapshot(w, g, R, K0), name)
        R.set_contact_feedback(0)                    # ... and with it off the same batch runs
        R.advance(K0, 2, TPU, H)
        assert R.tick_log_count() == 2
    with pytest.raises(RuntimeError, match='0: off, 1: on'):
        g._chk(g.L.srbm_controller_set_contact_feedback(g.h, 2))
