"""The command schedule of a whole-controller rollout on the GPU (srbm_controller_set_commands, _get_commands, _get_/_set_command_state,
_get_command_record, _get_command_costs, _command_dev; csrc/srbm_command.hiph through bilevel-gait-gen_amd/controller_rollout.py): the command
path and the setter path write the same bytes, the host function's; a schedule that never comes into force and a removed setting leave no trace;
one rollout however it is driven, with an absolute event and a later relative one, against the schedule-free rollout in which the host calls the
cost setters before every update; the gait entry with its line-search candidates; the sign of what a walk command does; everything on at once.
The world is test_gpu_controller_rollout.py's: 4 Config-B instances after one cold start, ticks of 10 ms; the rollouts on a ground are
contact_feedback_kit's, from tick 20."""
import numpy as np
import pytest

import command_kit as cmk
import contact_feedback_kit as ck
import controller_rollout_kit as kit
import sensors_kit as sk
import wb_joint_plant_kit as jk
import wb_terrain_plant_kit as tk
from gpu_kit import same_bytes
from srbm_loader import commands as cm
from srbm_loader import host, sensors
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS as F, COMMAND_RECORD_FIELDS as CF, PLANT_TORQUE_DRIVEN
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same
from test_gpu_wb_ground_plant import Rollouts, ground_snapshot
from test_gpu_wb_joint_plant import rollout_fresh

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


def base_costs(cfg):
    """Q[B][144] (= Phi) and des[12] of the cold start (host.BatchMPC.__init__)"""
    Q, des = host._tracking_cost(cfg)
    return np.tile(Q.reshape(1, 144), (B, 1)), des


def setter_costs(g, des, Q, Phi_w):
    """the setter path: srbm_add_quadratic_tracking_cost_each with des, srbm_set_linear_final_cost_each with Phi_w"""
    g.add_quadratic_tracking_cost_each(0, des, np.asarray(Q).reshape(-1, 12, 12))
    g.set_linear_final_cost_each(0, Phi_w)


# ---- 1. two paths, one set of bytes ----
def test_the_command_path_and_the_setter_path_write_the_bytes_of_the_host_function(world):
    """per-instance Q (the last one full) and Phi != Q; events per instance: an absolute one with a lead and rates, and a relative one in force at
    a second time.  srbm_controller_command_dev -> srbm_controller_get_command_costs against the _each setters called with the host function's
    des12 and Phi_w12 on a second batch, both against the host function; then srbm_export_qp's q of two instances; then the device's state and
    record against the host function's (field 6, a square root, within one unit in the last place: the device's documented bound for it; the
    rest, the sum of the squares included, byte for byte)"""
    L = host.lib()
    Q, Phi = cmk.cost_matrices(B)
    rng = np.random.default_rng(41)
    cmds = np.array([[cmk.event(0.1, rng.normal(size=12), rng.normal(size=12) * 0.3, lead=0.05),
                      cmk.event(0.4, rng.normal(size=12) * 0.1, rng.normal(size=12) * 0.3, lead=0.02, relative=True)] for b in range(B)])
    times = np.array([[0.23] * B, [0.41] * B, [0.47] * B])
    states = cmk.host_states(3, B, seed=43)
    want = cm.targets(L, cmds, Q, Phi, times, states)
    assert want['in_force'].all() and np.all(want['crec'][:, CF['events_begun']] == 2)
    ga, gb = world.base.clone(), world.base.clone()
    for g in (ga, gb):
        g.add_quadratic_tracking_cost_each(0, np.zeros((B, 12)), Q.reshape(B, 12, 12))
        g.set_quadratic_final_cost_each(0, Phi.reshape(B, 12, 12))
    Ra, Rb = ControllerRollout(ga), ControllerRollout(gb)
    Ra.set_commands(cmds)
    same_bytes(Ra.commands(), cmds, 'the schedule as set')
    t, s = Dev(times[0]), Dev(states[0])
    for u in range(3):
        t.put(times[u]); s.put(states[u])
        Ra.command_dev(t.p.value, s.p.value)
        wa, pa = Ra.command_costs()
        setter_costs(gb, want['des12'][u], Q, want['Phi_w12'][u])
        wb, pb = Rb.command_costs()
        for got, name in ((wa, 'command'), (wb, 'setters')):
            same_bytes(got, want['w12'][u], 'update %d: w, %s path' % (u, name))
        for got, name in ((pa, 'command'), (pb, 'setters')):
            same_bytes(got, want['Phi_w12'][u], 'update %d: Phi_w, %s path' % (u, name))
        if u == 0:
            for inst in (0, B - 1):
                qa, qb = ga.export_qp(inst)[-1], gb.export_qp(inst)[-1]
                same_bytes(qa, qb, 'q of instance %d' % inst)
                assert np.abs(qa - world.base.clone().export_qp(inst)[-1]).max() > 1e-3
    same_bytes(Ra.command_state(), want['cstate'], 'command state')
    crec = Ra.command_record()
    exact = [i for i in range(32) if i != CF['max_distance']]
    same_bytes(crec[:, exact], want['crec'][:, exact], 'command record')
    assert np.all(np.abs(crec[:, 6] - want['crec'][:, 6]) <= np.spacing(want['crec'][:, 6])) and np.all(crec[:, 6] > 0)
    # the state can be set and read; srbm_wb_plant_set_state re-initialises state and record
    cs = want['cstate'].copy(); cs[:, 1] += 0.25
    Ra.set_command_state(cs)
    same_bytes(Ra.command_state(), cs, 'command state as set')
    Ra.set_state(world.q, world.v)
    cs0, cr0 = cm.initial_state(B)
    same_bytes(Ra.command_state(), cs0, 'state after set_state'); same_bytes(Ra.command_record(), cr0, 'record after set_state')
    ga.close(); gb.close()


def test_refusals_of_the_setting_leave_the_one_in_force(world):
    g = world.base.clone()
    R = ControllerRollout(g)
    with pytest.raises(RuntimeError, match='srbm_controller_get_command_record: no command schedule is set'):
        R.command_record()
    with pytest.raises(RuntimeError, match='srbm_controller_get_command_state: no command schedule is set'):
        R.command_state()
    assert R.commands().shape == (B, 0, 28)
    _, des = base_costs(world.cfg)
    good = cm.stack([[cm.hold(0.1, des), cm.walk(0.3, 0.2, 0.0, world.cfg['mass'], des)]], batch=B)
    R.set_commands(good)
    for field, value, text in ((0, np.nan, 'must be finite'), (20, np.inf, 'must be finite'), (0, 0.05, 'must ascend'), (1, 2.0, 'must be 0 or 1'),
                               (2, -0.1, 'must be >= 0'), (3, 1.0, 'must be 0')):
        bad = good.copy(); bad[2, 1, field] = value
        with pytest.raises(RuntimeError, match=r'srbm_controller_set_commands: instance 2, event 1, field %d \(.*\): %s' % (field, text)):
            R.set_commands(bad)
        same_bytes(R.commands(), good, 'the schedule after the refused call')
    with pytest.raises(RuntimeError, match='srbm_controller_set_commands: n_events 9'):
        R.set_commands(np.zeros((B, 9, 28)))
    assert g.L.srbm_controller_set_commands(None, None, 0) != 0 and b'srbm_controller_set_commands' in g.L.srbm_last_error()
    with pytest.raises(RuntimeError, match='srbm_controller_set_command_state: instance 1: the latched index'):
        R.set_command_state(np.array([[-1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0.0]]))
    R.set_commands(good[0])                  # one schedule for every instance
    same_bytes(R.commands(), good, 'one schedule broadcast')
    g.close()


# ---- 2. transparency ----
@pytest.mark.parametrize('surface', SURFACES)
def test_a_schedule_beyond_the_rollout_is_the_rollout_without_the_setting_byte_for_byte(world, rollouts, surface):
    w, ro = world, rollouts
    _, des = base_costs(w.cfg)
    far = cm.stack([[cm.walk(100.0, 0.3, 0.1, w.cfg['mass'], des, lead=0.1), cm.hold(200.0, des + 1.0)]], batch=B)
    runs = []
    for on in (False, True):
        g, R = rollout_fresh(w, ro, surface, tick_log=NT, step_log=4)
        if on:
            R.set_commands(far)
        R.advance(0, NT, TPU, H)
        s = ground_snapshot(w, g, R, NT)
        s['tick_log'], s['step_log'] = R.tick_log(), g.step_log()
        s['w'], s['Phi_w'] = R.command_costs()
        runs.append(s)
    assert g.step_log_count() == 1
    assert_same(runs[0], runs[1], '%s: a schedule beyond the rollout against the setting off' % surface)
    cs0, cr0 = cm.initial_state(B)
    same_bytes(R.command_state(), cs0, 'state'); same_bytes(R.command_record(), cr0, 'record')


# ---- 3. one rollout however it is driven ----
K0, NTR, TPUR = 20, 12, 2
T_ABS, T_REL = 0.215, 0.25          # event 0 begins between the updates of ticks 20 and 22, event 1 between those of ticks 24 and 26
LATCH = 26


def rollout_schedule(cfg):
    """per instance: from 0.215 s the cold start's target shifted by a few centimetres, from 0.25 s a walk from where the robot then is (x and y of
    its des12 are 0: an offset of nothing from the anchor) with a lead of 50 ms"""
    _, des = base_costs(cfg)
    rel = des.copy(); rel[:2] = 0.0
    ev = []
    for b in range(B):
        shifted = des.copy(); shifted[0] += 0.02 * (b + 1); shifted[1] -= 0.01 * b
        ev.append([cm.hold(T_ABS, shifted), cm.walk(T_REL, 0.2 + 0.05 * b, 0.03 * (b - 1), cfg['mass'], rel, lead=0.05)])
    return cm.stack(ev)


class CommandWorld:
    """kind 1 on a flat ground, contact feedback on, 4 sub-steps, from tick 20 (contact_feedback_kit's world), the schedule above"""

    def __init__(self, w):
        self.w, self.gw = w, ck.GroundWorld(w)
        self.ground = ck.flat_ground(self.gw, K0)
        self.cmds = rollout_schedule(w.cfg)
        self.Q, _ = base_costs(w.cfg)

    def fresh(self, cmds='own', **kw):
        g, R = self.gw.fresh(K0, self.ground, feedback=1, **kw)
        if cmds is not None:
            R.set_commands(self.cmds if isinstance(cmds, str) else cmds)
        return g, R

    def snap(self, g, R, next_tick=K0 + NTR, commands=True):
        s = ck.ground_snapshot(snapshot, self.w, g, R, next_tick)
        s['w'], s['Phi_w'] = R.command_costs()
        if commands:
            s['cstate'], s['crec'] = R.command_state(), R.command_record()
        return s


def is_update(k, tpu=TPUR):
    return k > 0 and k % tpu == 0


def test_one_call_per_tick_calls_cuts_the_host_driven_chain_a_clone_and_the_setter_chain_end_on_the_same_bytes(world):
    w = world
    cw = CommandWorld(w)
    n_upd = NTR // TPUR
    ga, Ra = cw.fresh(tick_log=NTR, step_log=n_upd)
    Ra.advance(K0, NTR, TPUR, H)
    sa = cw.snap(ga, Ra)
    log, slog = Ra.tick_log(), ga.step_log()
    assert not ga.status()[1].any()
    # the record says what the schedule says: updates at ticks 20, 22 .. 30; none in force at 20, event 0 at 22 and 24, event 1 from 26
    rec = sa['crec']
    assert np.all(rec[:, CF['updates']] == 5) and np.all(rec[:, CF['index']] == 1) and np.all(rec[:, CF['events_begun']] == 2)
    assert np.all(rec[:, CF['latch_time']] == LATCH * H) and np.all(sa['cstate'][:, 0] == 1) and np.all(rec[:, CF['max_distance']] > 0)
    same_bytes(rec[:, CF['anchor']], sa['cstate'][:, 1:3], 'the anchor of the record is the state\'s')
    assert np.all(np.abs(rec[:, CF['anchor']] - log[LATCH - K0][:, F['base_pose']][:, :2]) < 0.05)          # near where the base was at the latch
    # ... and the schedule matters
    g0, R0 = cw.fresh(cmds=None, tick_log=NTR, step_log=n_upd)
    R0.advance(K0, NTR, TPUR, H)
    assert np.abs(R0.state()[0] - sa['q']).max() > 1e-6
    # one call per tick
    gb, Rb = cw.fresh(tick_log=NTR, step_log=n_upd)
    for k in range(K0, K0 + NTR):
        Rb.advance(k, 1, TPUR, H)
    assert_same(sa, cw.snap(gb, Rb), 'one call per tick against one call')
    same_bytes(Rb.tick_log(), log, 'tick log'); same_bytes(gb.step_log(), slog, 'step log')
    # a cut between the two events (after tick 23) and one between the latch (tick 26) and the next update (tick 28)
    gc, Rc = cw.fresh(tick_log=NTR, step_log=n_upd)
    Rc.advance(K0, 4, TPUR, H)
    assert np.all(Rc.command_state()[:, 0] == 0)
    Rc.advance(K0 + 4, 3, TPUR, H)
    assert np.all(Rc.command_state()[:, 0] == 1)
    Rc.advance(K0 + 7, NTR - 7, TPUR, H)
    assert_same(sa, cw.snap(gc, Rc), '4 + 3 + 5 ticks against one call')
    same_bytes(Rc.tick_log(), log, 'tick log: 4 + 3 + 5'); same_bytes(gc.step_log(), slog, 'step log: 4 + 3 + 5')
    # the chain of the device entries, driven from the host, with the command entry in its place; it keeps the states handed to the updates
    gd, Rd = cw.fresh(step_log=n_upd)
    q, v, _ = cw.gw.start(K0)
    T = ControlTick(gd)
    d = dict(q=Dev(q), v=Dev(v), cs=Dev(np.zeros((B, 4, 3))), t=Dev(np.zeros(B)), control=Dev(np.zeros((B, 36))), qp_sol=Dev(np.zeros((B, 30))),
             status=Dev(np.zeros((B, 2), np.int32)), contact=Dev(np.zeros((B, 4), np.int32)), state=Dev(np.zeros((B, 13))), ee=Dev(np.zeros((B, 4, 3))))
    upd_times, upd_states = [], []
    for k in range(K0, K0 + NTR):
        gd.synchronize()
        d['t'].put(np.full(B, k * H))
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        if is_update(k):
            Rd.contact_feedback_dev(d['t'].p.value, d['cs'].p.value)
            Rd.command_dev(d['t'].p.value, d['state'].p.value)
            gd.synchronize()
            upd_times.append(np.full(B, k * H)); upd_states.append(d['state'].get())
        Rd.ground_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['control'].p.value, d['status'].p.value)
        if is_update(k):
            gd.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
    gd.synchronize()
    cstate_d, crec_d = Rd.command_state(), Rd.command_record()
    Rd.set_state(d['q'].get(), d['v'].get()); Rd.set_contact_state(d['cs'].get())          # (set_state re-initialises state and record: they were read first)
    sd = cw.snap(gd, Rd)
    sd['cstate'], sd['crec'] = cstate_d, crec_d
    assert_same(sa, sd, 'the host-driven chain against one call')
    same_bytes(gd.step_log(), slog, 'step log: the chain')
    # the host function on the states the updates were handed: the same targets, state and record (field 6 within one unit in the last place)
    want = cm.targets(host.lib(), cw.cmds, cw.Q, cw.Q, np.array(upd_times), np.array(upd_states))
    assert want['in_force'][:, 0].tolist() == [False, True, True, True, True, True]
    same_bytes(sa['cstate'], want['cstate'], 'state against the host function')
    exact = [i for i in range(32) if i != CF['max_distance']]
    same_bytes(rec[:, exact], want['crec'][:, exact], 'record against the host function')
    assert np.all(np.abs(rec[:, 6] - want['crec'][:, 6]) <= np.spacing(want['crec'][:, 6]))
    same_bytes(sa['w'], want['w12'][-1], 'w after the last update'); same_bytes(sa['Phi_w'], want['Phi_w12'][-1], 'Phi_w after the last update')
    # a clone taken after the latch and continued
    ge, Re = cw.fresh()
    Re.advance(K0, 7, TPUR, H)
    ge.synchronize()
    twin = ge.clone()
    Rt = ControllerRollout(twin)
    same_bytes(Rt.command_state(), Re.command_state(), 'state of the clone'); same_bytes(Rt.command_record(), Re.command_record(), 'record of the clone')
    same_bytes(Rt.commands(), cw.cmds, 'the setting of the clone')
    assert np.all(Rt.command_state()[:, 0] == 1)
    Rt.advance(K0 + 7, NTR - 7, TPUR, H)
    assert_same(sa, cw.snap(twin, Rt), 'the clone made after the latch against the uncut run')
    # the relative event replaced by the absolute one built from the anchor of the record (x and y of the relative event's des12 are 0, so
    # (0 + p) + anchor and anchor + p are one sum)
    absolute = cw.cmds.copy()
    absolute[:, 1, 1] = 0.0
    absolute[:, 1, 4:6] = rec[:, CF['anchor']]
    gf, Rf = cw.fresh(cmds=absolute, tick_log=NTR, step_log=n_upd)
    Rf.advance(K0, NTR, TPUR, H)
    sf = cw.snap(gf, Rf)
    assert np.all(sf['crec'][:, CF['anchor']] == 0) and np.all(sf['cstate'][:, 1:3] == 0)
    keep = [i for i in range(32) if i not in (4, 5)]
    same_bytes(sf['crec'][:, keep], rec[:, keep], 'record of the absolute twin')
    sf_, sa_ = ({k: v for k, v in s.items() if k not in ('cstate', 'crec')} for s in (sf, sa))
    assert_same(sa_, sf_, 'the absolute event built from the anchor against the relative one')
    same_bytes(Rf.tick_log(), log, 'tick log: the absolute twin'); same_bytes(gf.step_log(), slog, 'step log: the absolute twin')
    # no schedule: the host calls the two _each setters with the host function's targets before every update
    gg, Rg = cw.fresh(cmds=None, tick_log=NTR, step_log=n_upd)
    u = 0
    for k in range(K0, K0 + NTR):
        if is_update(k):
            if want['in_force'][u, 0]:
                setter_costs(gg, want['des12'][u], cw.Q, want['Phi_w12'][u])
            u += 1
        Rg.advance(k, 1, TPUR, H)
    sg = cw.snap(gg, Rg, commands=False)
    assert_same({k: sa[k] for k in sg}, sg, 'the setter chain against the schedule')
    same_bytes(Rg.tick_log(), log, 'tick log: the setter chain'); same_bytes(gg.step_log(), slog, 'step log: the setter chain')
    # a schedule set, used and removed: the costs on the device are the host's base costs again
    Ra.set_commands(None)
    same_bytes(np.concatenate(Ra.command_costs()), np.concatenate(R0.command_costs()), 'costs after the setting was removed')
    assert np.abs(sa['w'] - R0.command_costs()[0]).max() > 1e-3


# ---- 4. the gait entry ----
def test_the_gait_entry_writes_the_candidates_costs_too(world):
    """srbm_gait_controller_advance, gait_opt_freq 3 on an update every 2 ticks from tick 20: gradient runs at ticks 22 and 28, line searches at
    24 (event 0 in force) and 30 (event 1).  One call against one call per tick, and against the schedule-free rollout in which the host calls
    the setters before every update with what the commanded run wrote (the des of its record, its Phi_w): a line search on stale candidate
    costs would differ"""
    w = world
    cw = CommandWorld(w)
    n_upd = NTR // TPUR
    ga, Ra = cw.fresh(tick_log=NTR, step_log=n_upd)
    gait_a = host.BatchGaitOptimizer(ga)
    Ra.advance(K0, NTR, TPUR, H, gait=gait_a, gait_opt_freq=3)
    sa = cw.snap(ga, Ra)
    log, slog = Ra.tick_log(), ga.step_log()
    gb, Rb = cw.fresh(tick_log=NTR, step_log=n_upd)
    gait_b = host.BatchGaitOptimizer(gb)
    written = {}
    for k in range(K0, K0 + NTR):
        Rb.advance(k, 1, TPUR, H, gait=gait_b, gait_opt_freq=3)
        if is_update(k) and Rb.command_record()[0, CF['updates']] > 0:
            written[k] = (Rb.command_record()[:, CF['des']], Rb.command_costs())
    assert sorted(written) == [22, 24, 26, 28, 30]
    assert_same(sa, cw.snap(gb, Rb), 'the gait entry: one call per tick against one call')
    same_bytes(Rb.tick_log(), log, 'the gait entry: tick log'); same_bytes(gb.step_log(), slog, 'the gait entry: step log')
    gc, Rc = cw.fresh(cmds=None, tick_log=NTR, step_log=n_upd)
    gait_c = host.BatchGaitOptimizer(gc)
    for k in range(K0, K0 + NTR):
        if k in written:
            des, (wk_, pw) = written[k]
            setter_costs(gc, des, cw.Q, pw)
            same_bytes(Rc.command_costs()[0], wk_, 'tick %d: w of the setter' % k)
        Rc.advance(k, 1, TPUR, H, gait=gait_c, gait_opt_freq=3)
    sc = cw.snap(gc, Rc, commands=False)
    assert_same({k: sa[k] for k in sc}, sc, 'the gait entry: the setter chain against the schedule')
    same_bytes(Rc.tick_log(), log, 'the gait entry: tick log of the setter chain'); same_bytes(gc.step_log(), slog, 'the gait entry: step log of the setter chain')
    ct_a, ct_c = gait_a.contact_times(), gait_c.contact_times()
    same_bytes(ct_a[0], ct_c[0], 'contact times'); assert np.array_equal(ct_a[1], ct_c[1])
    # the run holds line searches that searched, and the commands matter to it
    gd, Rd = cw.fresh(cmds=None, step_log=n_upd)
    gait_d = host.BatchGaitOptimizer(gd)
    Rd.advance(K0, NTR, TPUR, H, gait=gait_d, gait_opt_freq=3)
    assert np.abs(Rd.state()[0] - sa['q']).max() > 1e-6
    for x in (gait_a, gait_b, gait_c, gait_d):
        x.close()


# ---- 5. meaning: signs only ----
WALK_V = np.array([1.2, -1.2, 0.8, -0.8])
WALK_TICKS, WALK_T0, WALK_LEAD = 40, 0.2, 0.25


class TwinWorld:
    """four copies of instance 0 of the kit's world on its flat ground (kind 1, 4 sub-steps, contact feedback on) from tick 20: its cold start, its
    plant state, its ground.  Instance 0 is the one of the kit's four whose initial momenta leave it trotting in place in the uncommanded run (its x
    stays within 3 cm over the 40 ticks); the other three drift 0.17 m backwards in those 0.4 s, and what a command does to them is lost in that"""

    def __init__(self, w):
        self.w, gw = w, ck.GroundWorld(w)
        four = lambda a: np.tile(np.asarray(a)[:1], (B,) + (1,) * (np.ndim(a) - 1))
        self.base = host.BatchMPC.cold_start(w.cfg, four(w.states), four(w.ees))
        q, v, qd = gw.start(K0)
        self.q, self.v, self.qd, self.ground, self.act = four(q), four(v), four(qd), four(ck.flat_ground(gw, K0)), gw.act

    def fresh(self, cmds):
        g = self.base.clone()
        R = ControllerRollout(g)
        R.reset(self.qd)
        R.set_state(self.q, self.v)
        R.set_plant(PLANT_TORQUE_DRIVEN, *self.act, ck.SUB)
        R.set_ground(self.ground)
        R.set_contact_feedback(1)
        if cmds is not None:
            R.set_commands(cmds)
        return g, R


def test_a_walk_command_moves_the_base_its_way(world):
    """ticks 20 .. 59 of TwinWorld, an update every 5 ticks: four identical instances, commanded +1.2, -1.2, +0.8 and -0.8 m/s in one batch, against the
    same batch without the schedule (whose four instances end on the same bytes).  The walk is ABSOLUTE and starts from the cold start's own target,
    so that at v = 0 the commanded rollout is the uncommanded one and the difference is the motion alone (a relative walk also moves the target's x
    and y to where the robot stands: that alone shifted every instance of the kit's world by 1 to 2 cm in +x whatever the sign of v).
    The speeds are what this gait answers to within 0.4 s: measured on instance 0, at 0.2 m/s the displacement against the uncommanded run is of
    the size and of either sign of what any change of the costs does to the foot contacts (1 to 2 cm), from 0.4 m/s on its sign is the command's and
    it grows with the speed.  walk(+v) ends further in +x, walk(-v) further in -x, the four displacements are ordered as the four speeds are; record
    field 6 is positive and finite.  Signs and order only: the share of v * 0.4 s that is reached is a figure of DESIGN.md, not an assertion"""
    tw = TwinWorld(world)
    _, des = base_costs(world.cfg)
    cmds = cm.stack([[cm.walk(WALK_T0, v, 0.0, world.cfg['mass'], des, lead=WALK_LEAD, relative=False)] for v in WALK_V])
    ends = []
    for c in (None, cmds):
        g, R = tw.fresh(c)
        R.advance(K0, WALK_TICKS, TPU, H)
        assert not g.status()[1].any()
        ends.append(R.state()[0][:, 0])
    same_bytes(ends[0], np.full(B, ends[0][0]), 'the four uncommanded instances are one')
    moved = ends[1] - ends[0]
    rec = R.command_record()
    print('walk: speeds %s, base x against the uncommanded run after %.2f s %s m (v * stretch %s), record field 6 %s' % (
        WALK_V, WALK_TICKS * H, moved, WALK_V * WALK_TICKS * H, rec[:, 6]))
    assert np.all(moved[WALK_V > 0] > 0) and np.all(moved[WALK_V < 0] < 0), moved
    assert np.array_equal(np.argsort(moved), np.argsort(WALK_V)), moved
    assert np.all(rec[:, 6] > 0) and np.all(np.isfinite(rec[:, 6]))
    assert np.all(rec[:, CF['updates']] == 8) and np.all(rec[:, CF['events_begun']] == 1)
    g.close(); tw.base.close()


# ---- 6. with the rest on ----
def test_with_a_raised_terrain_contact_feedback_latency_and_sensors(world):
    """ticks 20 .. 31 on contact_feedback_kit.raised_ground as a terrain, an update every 3 ticks, latencies, sensors, the rollout's schedule (the
    relative event latches at tick 27): one call against a cut after the latch tick, byte for byte; the anchor is the MEASURED (x, y) of the latch
    tick, not the plant's"""
    gw = ck.GroundWorld(world)
    k0, tpu, nt, latch = K0, 3, NTR, 27
    lat = np.array([0.0, 0.012, 0.033, 0.0])
    sens, seed = sk.four_instances(H, sensors.record, sensors.lpf_x)
    ground = ck.raised_ground(gw, k0)
    cmds = rollout_schedule(world.cfg)
    runs = []
    for cut in (False, True):
        g, R = gw.fresh(k0, ground, feedback=1, tick_log=nt, step_log=4)
        R.set_terrain(tk.level_terrain(ground))
        R.set_latency(lat)
        R.set_sensors(sens, seed)
        R.set_commands(cmds)
        if cut:
            R.advance(k0, latch - k0 + 1, tpu, H)
            qm = R.measured()[0]
            anchor = R.command_state()[:, 1:3]
            same_bytes(anchor, qm[:, :2], 'the anchor is the measured (x, y) of the latch tick')
            truth = R.tick_log()[latch - k0][:, F['base_pose']][:, :2]
            assert np.any(anchor != truth)
            R.advance(latch + 1, k0 + nt - latch - 1, tpu, H)
        else:
            R.advance(k0, nt, tpu, H)
        g.synchronize()
        assert not g.status()[1].any()
        s = ck.ground_snapshot(snapshot, world, g, R, k0 + nt)
        s['feedback'], s['tick_log'], s['step_log'] = R.contact_feedback(), R.tick_log(), g.step_log()
        s['latency_record'], s['sensor_record'], s['measured'] = R.latency_record(), R.sensor_record(), np.concatenate(R.measured(), axis=1)
        s['cstate'], s['crec'] = R.command_state(), R.command_record()
        s['w'], s['Phi_w'] = R.command_costs()
        runs.append(s)
    assert_same(runs[0], runs[1], 'a cut after the latch against one call')
    assert np.all(runs[0]['crec'][:, CF['events_begun']] == 2) and np.all(runs[0]['crec'][:, CF['latch_time']] == latch * H)
