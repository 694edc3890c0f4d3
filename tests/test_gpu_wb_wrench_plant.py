"""The wrench schedule of the torque-driven whole-body plant on the GPU (srbm_wb_plant_set_wrenches, _get_wrenches, _get_wrench_record,
srbm_wb_wrench_force; csrc/srbm_wb_wrench.hiph through bilevel-gait-gen_amd/controller_rollout.py) against the restatement of
tests/wb_wrench_plant_kit.py, on held feet, ground and terrain, with and without a joint model: a schedule that never acts and a removed setting
are the plant without it byte for byte; the generalized force alone; the step with events that start and end inside a tick; the rollout cut in
every way, bit for bit, with the tick log's bit 4 where the host rule says; a shove and a payload; and everything on at once.  The world is
test_gpu_controller_rollout.py's: 4 Config-B instances after one cold start, ticks of 10 ms."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
import sensors_kit as sk
import wb_ground_plant_kit as gk
import wb_joint_plant_kit as jk
import wb_terrain_plant_kit as tk
import wb_torque_plant_kit as fd
import wb_wrench_plant_kit as wk
from gpu_kit import same_bytes
from srbm_loader import host, sensors
from srbm_loader import wrenches as wm
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS as F, FLAG_WRENCH, PLANT_QP_ACCELERATION, PLANT_TORQUE_DRIVEN
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same
from test_gpu_wb_ground_plant import cs_error, Rollouts, ground_snapshot
from test_gpu_wb_joint_plant import bare_plant, step_cases, set_surface, step_on_device, rollout_fresh, a1_joints

pytestmark = pytest.mark.gpu
B, H, TPU = kit.B, kit.TICK_DT, kit.TPU
NT = 10
SURFACES = (jk.HELD, jk.GROUND, jk.TERRAIN)


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def rollouts(world):
    return Rollouts(world)


def never_active(batch=B):
    """an empty slot, an event that is over before t = 0 and one that starts after every rollout here, per instance on other bodies"""
    return np.array([wk.pad([wk.event(0.0, 0.0, b), wk.event(-1.0, 0.5, 1 + b, (0.1, 0, 0), (50, 0, 0), (0, 1, 0), wk.BODY),
                             wk.event(100.0, wk.INF, 12 - b, (0, 0.1, 0), (0, 50, 0), (1, 0, 0))]) for b in range(batch)])


# ---- 1. a schedule that never acts, the setting removed, kind 0 ----
@pytest.mark.parametrize('surface', SURFACES)
def test_a_schedule_that_never_acts_is_the_plant_without_the_setting_byte_for_byte(world, rollouts, surface):
    """empty slots and events wholly outside the window, through the schedule's kernels, against the setting off, with and without a joint model:
    the step at S = 1 and 3 (q+, v+, (a, F) = sol_out, cs+, js+), and a logged NT-tick rollout (plant, cs, js, trajectories, q_des, both logs)"""
    cfg = world.cfg
    g, R, models, (kp, kd, lim) = bare_plant(cfg)
    W = never_active()
    js0 = np.random.default_rng(6).uniform(-3, 3, (B, 12))
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        cases = step_cases(surface, cfg, models)
        for rnd, (c, (J, stops)) in enumerate(zip(cases, jk.step_joints(cases))):
            set_surface(R, surface, c)
            for joints in (False, True):
                R.set_joints(J, stops) if joints else R.set_joints(None)
                res = []
                for on in (False, True):
                    R.set_wrenches(W if on else None)
                    if joints:
                        R.set_joint_state(js0)
                    out = step_on_device(g, R, surface, c, True)
                    res.append(out + ((R.joint_state(),) if joints else (None,)))
                for a, b, name in zip(res[0], res[1], ('q+', 'v+', '(a, F)', 'cs+', 'js+')):
                    if a is not None:
                        same_bytes(b, a, 'S %d round %d joints %s: %s' % (S, rnd, joints, name))
                wrec = R.wrench_record()
                assert np.all(wrec[:, 0] == S) and np.all(wrec[:, 1:] == 0)
    w, ro = world, rollouts
    J, _ = a1_joints()
    for joints in (False, True):
        runs = []
        for on in (False, True):
            g2, R2 = rollout_fresh(w, ro, surface, tick_log=NT, step_log=4)
            if joints:
                R2.set_joints(J, jk.A1_STOPS)
            if on:
                R2.set_wrenches(W)
            R2.advance(0, NT, TPU, H)
            s = ground_snapshot(w, g2, R2, NT)
            s['tick_log'], s['step_log'] = R2.tick_log(), g2.step_log()
            if joints:
                s['js'], s['jrec'] = R2.joint_state(), R2.joint_record()
            runs.append(s)
        assert_same(runs[0], runs[1], '%s, joints %s: the rollout with a schedule that never acts against the setting off' % (surface, joints))
        wrec = R2.wrench_record()
        assert np.all(wrec[:, 0] == NT * 4) and np.all(wrec[:, 1:] == 0)          # (Rollouts runs 4 sub-steps per tick)


def shoves(t0=0.015, d=0.05):
    return np.array([wk.pad([wk.event(t0, d, 0, (0.05, 0, 0.02), (0, 20.0 + 5 * b, 0), (0, 0, 0.5))]) for b in range(B)])


def test_a_schedule_removed_after_use_and_one_under_kind_0_leave_no_trace(world, rollouts):
    w, ro = world, rollouts
    ga, Ra = ro.fresh(tick_log=NT, step_log=4)
    Ra.set_wrenches(shoves())
    Ra.advance(0, 3, TPU, H)                 # used: no MPC update yet, so the trajectories are the start's
    wrec = Ra.wrench_record()
    assert np.all(wrec[:, 0] == 12) and np.all(wrec[:, 1] > 0) and np.all(wrec[:, 2] == 1) and np.all(wrec[:, 5] > 0)
    Ra.set_wrenches(None)
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_wrenches'):
        Ra.wrench_record()
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_wrenches'):
        Ra.wrenches()
    Ra.reset(w.q0); Ra.set_state(w.q, w.v); Ra.tick_log_reset()
    Ra.advance(0, NT, TPU, H)
    gb, Rb = ro.fresh(tick_log=NT, step_log=4)
    Rb.advance(0, NT, TPU, H)
    assert_same(ground_snapshot(w, ga, Ra, NT), ground_snapshot(w, gb, Rb, NT), 'a schedule set, used and removed against a batch that never had one')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    # kind 0 ignores the setting
    g0, R0 = w.fresh(tick_log=NT, step_log=4)
    R0.set_plant(PLANT_QP_ACCELERATION, *ro.act, 4)
    R0.set_wrenches(shoves(0.0, wk.INF))
    R0.advance(0, NT, TPU, H)
    g1, R1 = w.fresh(tick_log=NT, step_log=4)
    R1.advance(0, NT, TPU, H)
    assert_same(snapshot(w, g0, R0, NT), snapshot(w, g1, R1, NT), 'kind 0 with a schedule set against kind 0')
    same_bytes(R0.tick_log(), R1.tick_log(), 'tick log')
    assert np.all(R0.wrench_record() == 0)
    # what was set is what is returned; a refused setting leaves the one in force; set_state zeroes the record
    W = wk.force_cases(w.cfg)['W'][:B]
    R0.set_wrenches(W)
    same_bytes(R0.wrenches(), W, 'wrenches as set')
    bad = W.copy(); bad[2, 1, 2] = 13.0
    with pytest.raises(RuntimeError, match='instance 2, event 1, field 2'):
        R0.set_wrenches(bad)
    same_bytes(R0.wrenches(), W, 'wrenches after the refused call')
    with pytest.raises(RuntimeError, match='n_events 9'):
        R0.set_wrenches(np.zeros((B, 9, 16)))
    R0.set_wrenches(W[0])                    # one schedule for every instance
    same_bytes(R0.wrenches(), np.tile(W[0], (B, 1, 1)), 'one schedule broadcast')


# ---- 2. the generalized force alone ----
@pytest.mark.parametrize('large', (False, True))
def test_the_generalized_force_alone_against_the_restatement(large):
    """srbm_wb_wrench_force on wb_wrench_plant_kit.force_cases: 26 instances, one per (body, frame), a random posture, an off-origin point, force
    and torque; Q within 1e-9 max(1, |Q|_inf) of the kit's, the mask the host rule's; in both builds"""
    cfg = host.load_config('a1_configuration')
    c = wk.force_cases(cfg)
    n = len(c['q'])
    g = host.BatchMPC(dict(cfg, num_nodes=80) if large else cfg, n)
    assert (g.L is host.lib(True)) == large
    R = ControllerRollout(g)
    R.set_wrenches(c['W'])
    Q, mask = R.wrench_force(c['time'], c['q'])
    robot = kit.Model(cfg).robot
    worst = 0.0
    for b in range(n):
        m = wk.active_mask(c['W'][b], np.float64(c['time'][b]))
        assert m == 1 and mask[b] == m, (b, mask[b], m)
        want, _ = wk.generalized_force(robot, c['q'][b], c['W'][b], m)
        err = np.abs(Q[b] - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, err)
        assert err <= 1e-9 and np.abs(want).max() > 1.0, (b, err)
        if b >= 2:          # an event on a leg's body moves that leg's joints up to the body's own and no other joint
            ee, k = (b // 2 - 1) // 3, (b // 2 - 1) % 3
            live = np.zeros(12, bool); live[3 * ee:3 * ee + k + 1] = True
            assert np.all(Q[b, 6:][~live] == 0) and np.all(Q[b, 6:][live] != 0), b
        else:
            assert np.all(Q[b, 6:] == 0), b
    print('Q alone (%s build): worst %.3g relative' % ('LARGE' if large else 'standard', worst))
    # at a time at which no event is active: zero, mask 0; both events: mask 3
    Q0, m0 = R.wrench_force(c['time'] + 0.2, c['q'])
    assert not Q0.any() and not m0.any()
    W2 = c['W'].copy(); W2[:, 1, 0] = c['time'] - 0.01
    R.set_wrenches(W2)
    Q2, m2 = R.wrench_force(c['time'], c['q'])
    for b in (0, 7, 25):
        want, _ = wk.generalized_force(robot, c['q'][b], W2[b], 3)
        assert m2[b] == 3 and np.abs(Q2[b] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), b
    # the device entry on caller's arrays
    d = dict(t=Dev(c['time']), q=Dev(c['q']), Q=Dev(np.zeros((n, 18))), m=Dev(np.zeros(n, np.int32)))
    R.wrench_force_dev(d['t'].p.value, d['q'].p.value, d['Q'].p.value, d['m'].p.value)
    g.synchronize()
    same_bytes(d['Q'].get(), Q2, 'the device entry'); assert np.array_equal(d['m'].get(), m2)
    g.close()


# ---- 3. the step against the restatement ----
@pytest.mark.parametrize('surface', SURFACES)
def test_the_step_with_events_inside_the_tick_against_the_restatement(world, surface):
    """srbm_wb_fd_step_dev / srbm_wb_ground_step_dev (ground, terrain) with wb_wrench_plant_kit.step_schedule, the joint model on and off, at S = 1
    and S = 4, every round with its push: events on three bodies per instance, one in the body frame, one that starts and one that ends strictly
    inside a tick between sub-step times, an instance with its actuators off.  q+, v+, (a, F), js+ within 1e-9 (the step tests' bounds), the flags
    of cs+ equal and its anchors within 1e-9; the record's fields 0..2 exact, 3..6 within 1e-9"""
    cfg = world.cfg
    ctrl = kit.Model(cfg)
    g, R, models, (kp, kd, lim) = bare_plant(cfg)
    L = host.lib()
    js0 = np.random.default_rng(5).uniform(-3, 3, (B, 12))
    worst = 0.0
    for S in (1, 4):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        cases = step_cases(surface, cfg, models)
        assert tuple(c['k'] for c in cases) == wk.STEP_TICKS
        # from the host rule: EVERY instance has a sub-step with an event active and one without (over the rounds at S = 1, in every tick at S = 4)
        masks = np.concatenate([wm.active(L, wk.step_schedule(c['k'], H, S), c['k'], 1, H, S)[0] for c in cases])
        assert np.all((masks != 0).any(axis=0)) and np.all((masks == 0).any(axis=0)), masks
        limp = np.zeros(B, bool)
        for rnd, (c, (J, stops)) in enumerate(zip(cases, jk.step_joints(cases))):
            set_surface(R, surface, c)
            W = wk.step_schedule(c['k'], H, S)
            off = (c['status'][:, 1] & 255) > 1
            limp |= off
            if S == 4:
                m = wm.active(L, W, c['k'], 1, H, S)[0]
                assert np.all((m != 0).any(axis=0)) and np.all((m == 0).any(axis=0))
            for joints in (False, True):
                R.set_joints(J, stops) if joints else R.set_joints(None)
                R.set_wrenches(W)
                assert np.all(R.wrench_record() == 0)
                if joints:
                    R.set_joint_state(js0)
                q, v, sol, cs = step_on_device(g, R, surface, c, True)
                js, wrec = (R.joint_state() if joints else None), R.wrench_record()
                for b in range(B):
                    where = '%s S %d round %d instance %d joints %s' % (surface, S, rnd, b, joints)
                    qn, vn, csn, jsn, info = wk.wrench_step(surface, models[b], c['q'][b], c['v'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], W[b], H, S,
                                                            c['k'], ctrl.mass, ctrl.Ir_inv, (c['push_time'][b], c['impulse'][b]),
                                                            c['contact'][b] if surface == jk.HELD else None, c['cs'][b] if surface != jk.HELD else None,
                                                            c.get('ground', [None] * B)[b], c['terrain'][b] if surface == jk.TERRAIN else None,
                                                            J[b] if joints else None, stops[b], js0[b])
                    assert info['pushed'] == bool(c['want_push'][b]), where
                    errs = [np.abs(q[b] - qn).max(), np.abs(v[b] - vn).max(), np.abs(sol[b] - info['sol']).max() / max(1.0, np.abs(info['sol']).max())]
                    if joints:
                        errs.append(np.abs(js[b] - jsn).max())
                    if surface != jk.HELD:
                        cs_error(cs[b], csn, where)
                    want = wk.record_fold(np.zeros(8), S, H / S, info['history'])
                    assert np.array_equal(wrec[b, [0, 1, 2, 7]], want[[0, 1, 2, 7]]), (where, wrec[b], want)
                    errs.append(np.abs(wrec[b, 3:7] - want[3:7]).max())
                    worst = max(worst, max(errs))
                    assert max(errs) <= 1e-9, (where, errs)
        assert limp.any()
    print('%s: worst error %.3g' % (surface, worst))


# ---- 4. the rollout cut in every way ----
K0, NTR, TPUR, SUBR = 20, 12, 2, 4


def rollout_schedule():
    """ticks K0 .. K0 + NTR - 1 of 10 ms at 4 sub-steps: a shove on the trunk that starts strictly inside tick K0 + 2 and spans the cut after
    K0 + 4, a kick on a calf in the body frame inside ticks K0 + 8 and K0 + 9, an empty slot between them"""
    hs = H / SUBR
    return np.array([wk.pad([wk.event((K0 + 2) * H + 1.5 * hs, 4.2 * H, 0, (0.05, -0.02, 0.03), (3.0 * (b + 1), 10.0 + 4 * b, -2.0), (0.2, 0, 0.3)),
                             np.zeros(16),
                             wk.event((K0 + 8) * H + 0.3 * hs, 1.4 * H, 3 * (b + 1), (0, 0, -0.08), (6.0, -3.0, 1.0 + b), (0, 0.1, 0), wk.BODY)]) for b in range(B)])


class WrenchWorld:
    """kind 1 on a flat ground, contact feedback on, 4 sub-steps, from tick 20 (contact_feedback_kit's world), the schedule above"""

    def __init__(self, w):
        self.w, self.gw = w, ck.GroundWorld(w)
        self.ground = ck.flat_ground(self.gw, K0)
        self.W = rollout_schedule()

    def fresh(self, wrenches=True, **kw):
        g, R = self.gw.fresh(K0, self.ground, feedback=1, **kw)
        R.set_plant(PLANT_TORQUE_DRIVEN, *self.gw.act, SUBR)
        if wrenches:
            R.set_wrenches(self.W)
        return g, R

    def snap(self, g, R, next_tick=K0 + NTR):
        s = ck.ground_snapshot(snapshot, self.w, g, R, next_tick)
        s['wrec'] = R.wrench_record()
        return s


def test_one_call_one_call_per_tick_a_cut_the_host_driven_chain_the_gait_entry_and_a_clone_end_on_the_same_bytes(world):
    w = world
    ww = WrenchWorld(w)
    n_upd = NTR // TPUR
    ga, Ra = ww.fresh(tick_log=NTR, step_log=n_upd)
    Ra.advance(K0, NTR, TPUR, H)
    sa = ww.snap(ga, Ra)
    act = wm.active(host.lib(), ww.W, K0, NTR, H, SUBR)
    assert np.array_equal(sa['wrec'][:, 0], np.full(B, NTR * SUBR)) and np.array_equal(sa['wrec'][:, 1], (act != 0).sum(axis=(0, 1)))
    assert np.all(sa['wrec'][:, 2] == 5) and np.all(sa['wrec'][:, 3] > 0)
    # bit 4 of the flags on exactly the ticks the host rule predicts; the other bits are those of the rollout without the schedule
    log = Ra.tick_log()
    flags = log[:, :, F['flags']].astype(int)
    assert np.array_equal((flags & FLAG_WRENCH) != 0, (act != 0).any(axis=1)), flags
    assert ((flags & FLAG_WRENCH) != 0).any() and ((flags & FLAG_WRENCH) == 0).any()
    g0, R0 = ww.fresh(wrenches=False, tick_log=NTR)
    R0.advance(K0, NTR, TPUR, H)
    assert np.array_equal(flags & ~FLAG_WRENCH, R0.tick_log()[:, :, F['flags']].astype(int))
    assert np.abs(R0.state()[0] - sa['q']).max() > 1e-6             # the schedule matters
    # one call per tick; 5 + 7 with the shove spanning the cut
    gb, Rb = ww.fresh(tick_log=NTR, step_log=n_upd)
    for k in range(K0, K0 + NTR):
        Rb.advance(k, 1, TPUR, H)
    assert_same(sa, ww.snap(gb, Rb), 'one call per tick against one call')
    same_bytes(Rb.tick_log(), log, 'tick log'); same_bytes(gb.step_log(), ga.step_log(), 'step log')
    gc, Rc = ww.fresh(tick_log=NTR, step_log=n_upd)
    Rc.advance(K0, 5, TPUR, H); Rc.advance(K0 + 5, 7, TPUR, H)
    assert act[4].any() and act[5].any()
    assert_same(sa, ww.snap(gc, Rc), '5 + 7 ticks against one call')
    same_bytes(Rc.tick_log(), log, 'tick log: 5 + 7'); same_bytes(gc.step_log(), ga.step_log(), 'step log: 5 + 7')
    # the chain of the device entries, driven from the host; the step entry uses and advances the batch's record
    gd, Rd = ww.fresh(step_log=n_upd)
    q, v, _ = ww.gw.start(K0)
    T = ControlTick(gd)
    d = dict(q=Dev(q), v=Dev(v), cs=Dev(np.zeros((B, 4, 3))), t=Dev(np.zeros(B)), control=Dev(np.zeros((B, 36))), qp_sol=Dev(np.zeros((B, 30))),
             status=Dev(np.zeros((B, 2), np.int32)), contact=Dev(np.zeros((B, 4), np.int32)), state=Dev(np.zeros((B, 13))), ee=Dev(np.zeros((B, 4, 3))))
    for k in range(K0, K0 + NTR):
        gd.synchronize()
        d['t'].put(np.full(B, k * H))
        upd = k > 0 and k % TPUR == 0
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        if upd:
            Rd.contact_feedback_dev(d['t'].p.value, d['cs'].p.value)
        Rd.ground_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['control'].p.value, d['status'].p.value)
        if upd:
            gd.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
    gd.synchronize()
    wrec_d = Rd.wrench_record()
    Rd.set_state(d['q'].get(), d['v'].get()); Rd.set_contact_state(d['cs'].get())          # (set_state zeroes the record: it was read first)
    assert np.all(Rd.wrench_record() == 0)
    sd = ck.ground_snapshot(snapshot, w, gd, Rd, K0 + NTR)
    sd['wrec'] = wrec_d
    assert_same(sa, sd, 'the host-driven chain against one call')
    same_bytes(gd.step_log(), ga.step_log(), 'step log: the chain')
    # a clone taken mid-rollout, while the shove is on, and continued
    ge, Re = ww.fresh()
    Re.advance(K0, 5, TPUR, H)
    ge.synchronize()
    twin = ge.clone()
    Rt = ControllerRollout(twin)
    same_bytes(Rt.wrench_record(), Re.wrench_record(), 'wrec of the clone'); same_bytes(Rt.wrenches(), ww.W, 'the setting of the clone')
    Rt.advance(K0 + 5, NTR - 5, TPUR, H)
    assert_same(sa, ww.snap(twin, Rt), 'the clone made mid-rollout against the uncut run')
    # the gait entry: one call against one call per tick
    gf, Rf = ww.fresh(tick_log=NTR, step_log=n_upd)
    gait_f = host.BatchGaitOptimizer(gf)
    Rf.advance(K0, NTR, TPUR, H, gait=gait_f, gait_opt_freq=3)
    gh, Rh = ww.fresh(tick_log=NTR, step_log=n_upd)
    gait_h = host.BatchGaitOptimizer(gh)
    for k in range(K0, K0 + NTR):
        Rh.advance(k, 1, TPUR, H, gait=gait_h, gait_opt_freq=3)
    sf = ww.snap(gf, Rf)
    assert_same(sf, ww.snap(gh, Rh), 'the gait entry: one call per tick against one call')
    same_bytes(Rh.tick_log(), Rf.tick_log(), 'the gait entry: tick log'); same_bytes(gh.step_log(), gf.step_log(), 'the gait entry: step log')
    assert np.array_equal(sf['wrec'][:, :3], sa['wrec'][:, :3])
    assert np.array_equal((Rf.tick_log()[:, :, F['flags']].astype(int) & FLAG_WRENCH) != 0, (act != 0).any(axis=1))
    gait_f.close(); gait_h.close()


# ---- 5. meaning: signs only ----
SHOVE_T0, SHOVE_D, SHOVE_F = 0.051, 0.15, 60.0          # starts and ends strictly between two sub-step times: 60 sub-steps of 2.5 ms
PAYLOAD = 49.05


def test_a_shove_moves_the_base_its_way_and_a_payload_lowers_it(world):
    """three instances standing on a ground under their joint PD loops, ticks of 10 ms at S = 4 through srbm_wb_ground_step_dev: 0 undisturbed,
    1 with a +y 60 N world force on the trunk for 150 ms, 2 with 49.05 N downwards at the trunk's centre of mass from t = 0 for good.  The shoved
    instance within 1e-9 of the restatement over the first 30 ticks; at the end of the shove its base is more than 1e-4 m further in +y than the
    undisturbed one's; the loaded base ends lower; the record's impulse is F times the active time to 1e-9.  Signs only: no magnitude was measured"""
    cfg = world.cfg
    model = kit.Model(cfg)
    n, S, ticks, check = 3, 4, 30, 30
    q0 = np.array(cfg['init_config'], float)
    low = kit.ik.forward_kinematics(model.legs, q0)[:, 2].min()
    ground = gk.ground_params(low + 0.002, k_n=5000.0, d_n=60.0, mu=0.7, k_t=3000.0, d_t=40.0)
    kp, kd, lim = np.full(12, fd.KP), np.full(12, fd.KD), np.asarray(cfg['torque_bounds'], float)
    control = np.concatenate([q0[7:], np.zeros(24)])
    com = cfg['body_model'][0]['com']
    W = np.array([wk.pad([]), wk.pad([wk.event(SHOVE_T0, SHOVE_D, 0, (0, 0, 0), (0, SHOVE_F, 0))]), wk.pad([wk.event(0.0, wk.INF, 0, com, (0, 0, -PAYLOAD))])])
    g = host.BatchMPC(cfg, n)
    R = ControllerRollout(g)
    R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
    R.set_ground(ground)
    R.set_wrenches(W)
    d = dict(q=Dev(np.tile(q0, (n, 1))), v=Dev(np.zeros((n, 18))), cs=Dev(np.zeros((n, 4, 3))), ctl=Dev(np.tile(control, (n, 1))), st=Dev(np.zeros((n, 2), np.int32)))
    q, v, cs = q0, np.zeros(18), gk.NO_CONTACT
    worst, end_tick = 0.0, int((SHOVE_T0 + SHOVE_D) / H) + 1          # the first tick after the shove's last sub-step
    y_end = None
    for k in range(ticks):
        R.ground_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value)
        g.synchronize()
        qd = d['q'].get()
        if k < check:
            q, v, cs, _, _ = wk.wrench_step(jk.GROUND, model, q, v, control, False, kp, kd, lim, W[1], H, S, k, model.mass, model.Ir_inv, cs=cs, gr=ground)
            errs = [np.abs(qd[1] - q).max(), np.abs(d['v'].get()[1] - v).max()]
            cs_error(d['cs'].get()[1], cs, 'tick %d' % k)
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-9, (k, errs)
        if k == end_tick - 1:
            y_end = qd[1, 1] - qd[0, 1]
    wrec = R.wrench_record()
    act = wm.active(host.lib(), W, 0, ticks, H, S)
    n_act = (act != 0).sum(axis=(0, 1))
    print('shove: worst error over %d ticks %.3g; base y against undisturbed at the end of the shove %.4g m; payload: base z against undisturbed %.4g m' % (
        check, worst, y_end, qd[2, 2] - qd[0, 2]))
    assert n_act.tolist() == [0, int(round(SHOVE_D / (H / S))), ticks * S] and np.array_equal(wrec[:, 1], n_act)
    assert y_end > 1e-4
    assert qd[2, 2] < qd[0, 2]
    hs = H / S
    assert np.all(wrec[0, 1:] == 0)
    assert np.abs(wrec[1, 4:7] - np.array([0, SHOVE_F, 0]) * n_act[1] * hs).max() <= 1e-9
    assert np.abs(wrec[2, 4:7] - np.array([0, 0, -PAYLOAD]) * n_act[2] * hs).max() <= 1e-9
    g.close()


# ---- 6. everything on ----
def test_with_a_raised_terrain_contact_feedback_latency_sensors_and_the_gait_step(world):
    """ticks 20 .. 31 on contact_feedback_kit.raised_ground as a terrain, an update every 3, gait_opt_freq 5, latencies, sensors, the rollout's
    schedule: one call against one call per tick, byte for byte"""
    gw = ck.GroundWorld(world)
    k0, tpu, nt, freq = K0, 3, NTR, 5
    lat = np.array([0.0, 0.012, 0.033, 0.0])
    sens, seed = sk.four_instances(H, sensors.record, sensors.lpf_x)
    ground = ck.raised_ground(gw, k0)
    W = rollout_schedule()
    runs = []
    for per_tick in (False, True):
        g, R = gw.fresh(k0, ground, feedback=1, tick_log=nt, step_log=4)
        R.set_terrain(tk.level_terrain(ground))
        gait = host.BatchGaitOptimizer(g)
        R.set_latency(lat)
        R.set_sensors(sens, seed)
        R.set_wrenches(W)
        for a in (range(k0, k0 + nt) if per_tick else [k0]):
            R.advance(a, 1 if per_tick else nt, tpu, H, gait=gait, gait_opt_freq=freq)
        g.synchronize()
        assert not g.status()[1].any()
        s = ck.ground_snapshot(snapshot, world, g, R, k0 + nt)
        s['feedback'], s['tick_log'], s['step_log'], s['wrec'] = R.contact_feedback(), R.tick_log(), g.step_log(), R.wrench_record()
        s['latency_record'], s['sensor_record'], s['measured'] = R.latency_record(), R.sensor_record(), np.concatenate(R.measured(), axis=1)
        s['contact_times'], s['counts'] = gait.contact_times()
        runs.append(s)
        gait.close()
    assert_same(runs[0], runs[1], 'one call per tick against one call')
    act = wm.active(host.lib(), W, k0, nt, H, ck.SUB)
    assert np.array_equal(runs[0]['wrec'][:, 1], (act != 0).sum(axis=(0, 1))) and np.all(runs[0]['wrec'][:, 2] == 5)
