"""The joint model of the torque-driven whole-body plant on the GPU (srbm_wb_plant_set_joints, _get_joints, _get / _set_joint_state,
_get_joint_record; csrc/srbm_wb_joints.hiph through bilevel-gait-gen_amd/controller_rollout.py) against the restatement of
tests/wb_joint_plant_kit.py, on held feet, ground and terrain: the transparent model and the removed setting are the plant without it byte for byte;
the armature in the three solves; the step with every branch of the law; the rollout three ways, through the gait entry and as a clone cut
mid-rollout, bit for bit; a large armature and the limp drop.  The world is test_gpu_controller_rollout.py's: 4 Config-B instances after one cold
start, ticks of 10 ms, an MPC update every 5 ticks, instance 2 pushed in tick 3."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_joint_plant_kit as jk
import wb_terrain_plant_kit as tk
import wb_torque_plant_kit as fd
from gpu_kit import same_bytes
from srbm_loader import host
from srbm_loader import joints as jm
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, PLANT_QP_ACCELERATION, PLANT_TORQUE_DRIVEN
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same
from test_gpu_wb_ground_plant import own_bodies, cs_error, Rollouts, ground_snapshot

pytestmark = pytest.mark.gpu
B, H, TPU = kit.B, kit.TICK_DT, kit.TPU
NT = 10                 # ticks of the logged rollouts: the push in tick 3 and the MPC update after tick 5 are inside
SURFACES = (jk.HELD, jk.GROUND, jk.TERRAIN)


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def rollouts(world):
    return Rollouts(world)


def bare_plant(cfg, S=1):
    """a batch that never solved: kind 1, bodies of the plant's own on the odd instances, the step tests' actuators"""
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    lists, models = own_bodies(cfg)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    kp, kd, lim = fd.step_actuators(cfg)
    R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
    return g, R, models, (kp, kd, lim)


def step_cases(surface, cfg, models):
    cases = {jk.HELD: lambda: fd.step_cases(cfg, H), jk.GROUND: lambda: gk.step_cases(cfg, models, H), jk.TERRAIN: lambda: tk.step_cases(cfg, models, H)}[surface]()
    return jk.step_rates(cases)          # the rates the branches of the law need (wb_joint_plant_kit.step_joints)


def set_surface(R, surface, c):
    if surface == jk.HELD:
        R.set_ground(None)
        return
    R.set_ground(c['ground'])
    R.set_terrain(c['terrain'] if surface == jk.TERRAIN else None)


def step_on_device(g, R, surface, c, pushed):
    """-> q+, v+, (a, F), cs+ (None with the feet held)"""
    g.plant_set_push(c['push_time'], c['impulse']) if pushed else g.plant_set_push()
    d = dict(q=Dev(c['q']), v=Dev(c['v']), ctl=Dev(c['control']), st=Dev(c['status']), sol=Dev(np.zeros((B, 30))))
    if surface == jk.HELD:
        d['con'] = Dev(c['contact'])
        R.fd_step_dev(c['k'], H, d['q'].p.value, d['v'].p.value, d['ctl'].p.value, d['con'].p.value, d['st'].p.value, d['sol'].p.value)
    else:
        d['cs'] = Dev(c['cs'])
        R.ground_step_dev(c['k'], H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value, d['sol'].p.value)
    g.synchronize()
    return d['q'].get(), d['v'].get(), d['sol'].get(), d['cs'].get() if surface != jk.HELD else None


def rollout_fresh(w, ro, surface, **kw):
    g, R = ro.fresh(ground=surface != jk.HELD, **kw)
    if surface == jk.TERRAIN:
        R.set_terrain(tk.rollout_terrain(w.q, w.model.legs))
    return g, R


def a1_joints():
    return jm.a1_model(jk.load_fixture(), jk.A1_STICTION_BAND, jk.A1_MOTOR_T)


# ---- 1. the transparent model is the parent's bytes ----
@pytest.mark.parametrize('surface', SURFACES)
def test_the_transparent_model_is_the_plant_without_the_setting_byte_for_byte(world, rollouts, surface):
    """b = I_a = f_c = v_s = T = 0 and infinite ranges, through the joint model's kernels, against the setting off: the step at S = 1 and 3 with and
    without a push (q+, v+, (a, F), cs+), and a logged NT-tick rollout (plant, cs, trajectories, q_des, tick log, step log)"""
    cfg = world.cfg
    g, R, models, (kp, kd, lim) = bare_plant(cfg)
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        for rnd, c in enumerate(step_cases(surface, cfg, models)):
            set_surface(R, surface, c)
            for pushed in (False, True):
                R.set_joints(None)
                off = step_on_device(g, R, surface, c, pushed)
                R.set_joints(jk.transparent(), (100.0, 1.0))
                on = step_on_device(g, R, surface, c, pushed)
                for a, b, name in zip(off, on, ('q+', 'v+', '(a, F)', 'cs+')):
                    if a is not None:
                        same_bytes(b, a, 'S %d round %d pushed %s: %s' % (S, rnd, pushed, name))
                jrec = R.joint_record()
                assert np.all(jrec[:, 0] == S) and np.all(jrec[:, 1:] == 0)
                not_off = (c['status'][:, 1] & 255) <= 1
                assert np.any(R.joint_state()[not_off] != 0) and np.all(R.joint_state()[~not_off] == 0)        # T = 0: tau_m is the command
    w, ro = world, rollouts
    ga, Ra = rollout_fresh(w, ro, surface, tick_log=NT, step_log=4)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = rollout_fresh(w, ro, surface, tick_log=NT, step_log=4)
    Rb.set_joints(jk.transparent(B), (100.0, 1.0))
    Rb.advance(0, NT, TPU, H)
    assert_same(ground_snapshot(w, ga, Ra, NT), ground_snapshot(w, gb, Rb, NT), 'the rollout with the transparent model against the setting off')
    same_bytes(Rb.tick_log(), Ra.tick_log(), 'tick log')
    same_bytes(gb.step_log(), ga.step_log(), 'step log')
    jrec = Rb.joint_record()
    assert np.all(jrec[:, 0] == NT * 4) and np.all(jrec[:, 1:] == 0)          # (Rollouts runs 4 sub-steps per tick)


# ---- 2. the setting removed ----
def test_a_joint_model_removed_after_use_and_one_under_kind_0_leave_no_trace(world, rollouts):
    w, ro = world, rollouts
    J, lim = a1_joints()
    ga, Ra = ro.fresh(tick_log=NT, step_log=4)
    Ra.set_joints(J, jk.A1_STOPS)
    Ra.advance(0, 3, TPU, H)                 # used: no MPC update yet, so the trajectories are the start's
    assert np.any(Ra.joint_state() != 0) and np.all(Ra.joint_record()[:, 0] == 12)
    Ra.set_joints(None)
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_joints'):
        Ra.joint_state()
    Ra.reset(w.q0); Ra.set_state(w.q, w.v); Ra.tick_log_reset()
    Ra.advance(0, NT, TPU, H)
    gb, Rb = ro.fresh(tick_log=NT, step_log=4)
    Rb.advance(0, NT, TPU, H)
    assert_same(ground_snapshot(w, ga, Ra, NT), ground_snapshot(w, gb, Rb, NT), 'a joint model set, used and removed against a batch that never had one')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    # kind 0 ignores the setting
    g0, R0 = w.fresh(tick_log=NT, step_log=4)
    R0.set_plant(PLANT_QP_ACCELERATION, *ro.act, 4)
    R0.set_joints(J, jk.A1_STOPS)
    R0.advance(0, NT, TPU, H)
    g1, R1 = w.fresh(tick_log=NT, step_log=4)
    R1.advance(0, NT, TPU, H)
    assert_same(snapshot(w, g0, R0, NT), snapshot(w, g1, R1, NT), 'kind 0 with a joint model set against kind 0')
    same_bytes(R0.tick_log(), R1.tick_log(), 'tick log')
    assert np.all(R0.joint_record() == 0) and np.all(R0.joint_state() == 0)
    # what was set is what is returned; a refused setting leaves the one in force
    Jb = np.tile(J, (B, 1, 1)); Jb[1, 3, jk.JB] = 0.25
    R0.set_joints(Jb, [(150.0 + b, 1.0 * b) for b in range(B)])
    got, stops = R0.joints()
    same_bytes(got, Jb, 'joints as set'); assert np.array_equal(stops, [(150.0 + b, 1.0 * b) for b in range(B)])
    bad = Jb.copy(); bad[2, 7, jk.JVS] = 0.0
    with pytest.raises(RuntimeError, match='instance 2, joint 7, field 3'):
        R0.set_joints(bad, jk.A1_STOPS)
    same_bytes(R0.joints()[0], Jb, 'joints after the refused call')
    with pytest.raises(RuntimeError, match='instance 1, joint 4'):
        js = np.zeros((B, 12)); js[1, 4] = np.nan
        R0.set_joint_state(js)


# ---- 3. the armature in the solve ----
def test_the_armature_in_the_three_solves_against_the_restatement(world):
    """srbm_wb_forward_dynamics (every contact pattern) and srbm_wb_ground_dynamics on the ground and on a terrain (every branch of their laws) with
    I_a from 0 to 0.1 mixed within an instance, tau the net joint torque: (a, F) within 1e-9 max(1, |x|_inf) of np.linalg.solve on the restated
    system with I_a on the diagonal, the dynamics residual (with I_a a on the joint rows) within 1e-9 max(1, |tau|_inf) -- the bounds of
    test_gpu_wb_ground_plant.py -- and the armature matters"""
    cfg = world.cfg
    g, R, models, _ = bare_plant(cfg)
    J = jk.solve_armatures()
    worst = {}
    for surface in SURFACES:
        cases = {jk.HELD: lambda: [dict(q=q, v=v, tau=tau, contact=con) for q, v, tau, con in fd.solve_cases(cfg)],
                 jk.GROUND: lambda: gk.solve_cases(cfg, models), jk.TERRAIN: lambda: tk.solve_cases(cfg, models)}[surface]()
        wx = wr = 0.0
        for c, case in enumerate(cases):
            set_surface(R, surface, case)
            res = {}
            for on in (False, True):
                R.set_joints(J, (100.0, 1.0)) if on else R.set_joints(None)
                if surface == jk.HELD:
                    sol, st = R.forward_dynamics(case['q'], case['v'], case['tau'], case['contact'])
                    cs_out = None
                else:
                    sol, cs_out, st = R.ground_dynamics(case['q'], case['v'], case['tau'], case['cs'])
                assert np.all(st == 0), (surface, c, st)
                res[on] = (sol, cs_out)
            sol, cs_out = res[True]
            assert np.abs(res[True][0][:, :18] - res[False][0][:, :18]).max() > 1e-3
            for b in range(B):
                where = '%s call %d instance %d' % (surface, c, b)
                want, cs_want, _ = jk.dynamics(surface, models[b], J[b], case['q'][b], case['v'][b], case['tau'][b], case.get('contact', [None] * B)[b],
                                               case['cs'][b] if 'cs' in case else None, case['ground'][b] if 'ground' in case else None,
                                               case['terrain'][b] if 'terrain' in case else None)
                ex = np.abs(sol[b] - want).max() / max(1.0, np.abs(want).max())
                if surface == jk.HELD:
                    contact = case['contact'][b]
                    F = kit.unstack_forces(sol[b], contact)
                else:
                    contact, F = np.ones(4, int), sol[b, 18:].reshape(4, 3)
                    cs_error(cs_out[b], cs_want, where)
                r = jk.residual_with_armature(models[b], J[b], case['q'][b], case['v'][b], sol[b], case['tau'][b], F, contact)
                er = np.abs(r).max() / max(1.0, np.abs(case['tau'][b]).max())
                wx, wr = max(wx, ex), max(wr, er)
                assert ex <= 1e-9 and er <= 1e-9, (where, ex, er)
        worst[surface] = (wx, wr)
        print('%s: worst (a, F) %.3g relative, dynamics residual %.3g relative' % (surface, wx, wr))


# ---- 4. the step against the restatement ----
@pytest.mark.parametrize('surface', SURFACES)
def test_the_step_with_every_branch_of_the_law_against_the_restatement(world, surface):
    """srbm_wb_fd_step_dev / srbm_wb_ground_step_dev (ground, terrain) with wb_joint_plant_kit.step_joints at S = 1 and 3 from a motor state that is
    not zero: instance TABLE with the CPU test's kinds of joints, a joint that crosses its stop in sub-step 2 of 3, in the tick in which a foot touches
    down and one lifts off.  q+, v+, (a, F), js+ within 1e-9 (the step tests' bounds), the flags of cs+ equal and its anchors within 1e-9; the
    record's counts and mask exact, its maxima within 1e-9"""
    cfg = world.cfg
    ctrl = kit.Model(cfg)
    g, R, models, (kp, kd, lim) = bare_plant(cfg)
    js0 = np.random.default_rng(5).uniform(-3, 3, (B, 12))
    seen, crossed, worst = set(), False, 0.0
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        cases = step_cases(surface, cfg, models)
        for rnd, (c, (J, stops)) in enumerate(zip(cases, jk.step_joints(cases))):
            set_surface(R, surface, c)
            off = (c['status'][:, 1] & 255) > 1
            for pushed in (False, True):
                R.set_joints(J, stops)
                assert np.all(R.joint_state() == 0) and np.all(R.joint_record() == 0)
                R.set_joint_state(js0)
                q, v, sol, cs = step_on_device(g, R, surface, c, pushed)
                js, jrec = R.joint_state(), R.joint_record()
                for b in range(B):
                    where = '%s S %d round %d instance %d pushed %s' % (surface, S, rnd, b, pushed)
                    push = (c['push_time'][b], c['impulse'][b]) if pushed else None
                    qn, vn, csn, jsn, info = jk.joint_step(surface, models[b], c['q'][b], c['v'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], J[b], stops[b],
                                                           js0[b], H, S, c['k'], ctrl.mass, ctrl.Ir_inv, push, c['contact'][b] if surface == jk.HELD else None,
                                                           c['cs'][b] if surface != jk.HELD else None, c.get('ground', [None] * B)[b],
                                                           c['terrain'][b] if surface == jk.TERRAIN else None)
                    assert info['pushed'] == (pushed and bool(c['want_push'][b])), where
                    errs = [np.abs(q[b] - qn).max(), np.abs(v[b] - vn).max(), np.abs(sol[b] - info['sol']).max() / max(1.0, np.abs(info['sol']).max()),
                            np.abs(js[b] - jsn).max()]
                    if surface != jk.HELD:
                        cs_error(cs[b], csn, where)
                    want = jk.record_fold(np.zeros(8), *jk.fold_infos(info['history']))
                    assert np.array_equal(jrec[b, [0, 1, 5, 6, 7]], want[[0, 1, 5, 6, 7]]), (where, jrec[b], want)
                    errs.append(np.abs(jrec[b, 2:5] - want[2:5]).max())
                    worst = max(worst, max(errs))
                    assert max(errs) <= 1e-9, (where, errs)
                    seen |= {x for infos in info['history'] for i in infos for x in i['branch']}
                    if S == 3 and b == jk.CROSSING[0]:
                        e = [infos[jk.CROSSING[1]]['exc'] for infos in info['history']]
                        crossed |= e[0] == 0 and e[1] > 0
                    if off[b]:          # the actuators are off: a motor without lag is at 0, one with a lag decays
                        assert np.all(js[b][J[b][:, jk.JT] == 0] == 0), where
    print('%s: worst error %.3g; branches taken %s' % (surface, worst, sorted(seen)))
    assert seen == {'lag', 'damped', 'band', 'sat+', 'sat-', 'lower', 'lower-clamped', 'upper', 'upper-clamped'} and crossed


# ---- 5. the rollout three ways, the gait entry, the clone ----
K0, NTR, TPUR, SUBR = 20, 12, 2, 3


class JointWorld:
    """kind 1 on a flat ground with the A1 fixture's joint values, contact feedback on, 3 sub-steps, from tick 20 (contact_feedback_kit's world)"""

    def __init__(self, w):
        self.w, self.gw = w, ck.GroundWorld(w)
        self.ground = ck.flat_ground(self.gw, K0)
        self.J, self.lim = a1_joints()

    def fresh(self, **kw):
        g, R = self.gw.fresh(K0, self.ground, feedback=1, **kw)
        R.set_plant(PLANT_TORQUE_DRIVEN, self.gw.act[0], self.gw.act[1], np.tile(self.lim, (B, 1)), SUBR)
        R.set_joints(self.J, jk.A1_STOPS)
        return g, R

    def snap(self, g, R, next_tick=K0 + NTR):
        s = ck.ground_snapshot(snapshot, self.w, g, R, next_tick)
        s['js'], s['jrec'] = R.joint_state(), R.joint_record()
        return s


def test_one_call_one_call_per_tick_the_host_driven_chain_the_gait_entry_and_a_clone_end_on_the_same_bytes(world):
    w = world
    jw = JointWorld(w)
    n_upd = NTR // TPUR
    ga, Ra = jw.fresh(tick_log=NTR, step_log=n_upd)
    Ra.advance(K0, NTR, TPUR, H)
    sa = jw.snap(ga, Ra)
    assert np.all(sa['jrec'][:, 0] == NTR * SUBR) and np.all(sa['jrec'][:, 3] > 0) and np.all(sa['jrec'][:, 4] > 0) and np.any(sa['js'] != 0)
    gb, Rb = jw.fresh(tick_log=NTR, step_log=n_upd)
    for k in range(K0, K0 + NTR):
        Rb.advance(k, 1, TPUR, H)
    assert_same(sa, jw.snap(gb, Rb), 'one call per tick against one call')
    same_bytes(Rb.tick_log(), Ra.tick_log(), 'tick log')
    same_bytes(gb.step_log(), ga.step_log(), 'step log')
    # the chain of the device entries, driven from the host; the step entry uses and advances the batch's js and jrec
    gc, Rc = jw.fresh(step_log=n_upd)
    q, v, _ = jw.gw.start(K0)
    T = ControlTick(gc)
    d = dict(q=Dev(q), v=Dev(v), cs=Dev(np.zeros((B, 4, 3))), t=Dev(np.zeros(B)), control=Dev(np.zeros((B, 36))), qp_sol=Dev(np.zeros((B, 30))),
             status=Dev(np.zeros((B, 2), np.int32)), contact=Dev(np.zeros((B, 4), np.int32)), state=Dev(np.zeros((B, 13))), ee=Dev(np.zeros((B, 4, 3))))
    for k in range(K0, K0 + NTR):
        gc.synchronize()
        d['t'].put(np.full(B, k * H))
        upd = k > 0 and k % TPUR == 0
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        if upd:
            Rc.contact_feedback_dev(d['t'].p.value, d['cs'].p.value)
        Rc.ground_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['control'].p.value, d['status'].p.value)
        if upd:
            gc.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
    gc.synchronize()
    js_c, jrec_c = Rc.joint_state(), Rc.joint_record()
    Rc.set_state(d['q'].get(), d['v'].get()); Rc.set_contact_state(d['cs'].get())          # (set_state resets js and jrec: they were read first)
    assert np.all(Rc.joint_state() == 0) and np.all(Rc.joint_record() == 0)
    sc = ck.ground_snapshot(snapshot, w, gc, Rc, K0 + NTR)
    sc['js'], sc['jrec'] = js_c, jrec_c
    assert_same(sa, sc, 'the host-driven chain against one call')
    same_bytes(gc.step_log(), ga.step_log(), 'step log: the chain')
    # a clone taken mid-rollout and continued, against the uncut run
    gd, Rd = jw.fresh()
    Rd.advance(K0, 5, TPUR, H)
    gd.synchronize()
    twin = gd.clone()
    Rt = ControllerRollout(twin)
    same_bytes(Rt.joint_state(), Rd.joint_state(), 'js of the clone'); same_bytes(Rt.joint_record(), Rd.joint_record(), 'jrec of the clone')
    same_bytes(Rt.joints()[0], Rd.joints()[0], 'the setting of the clone')
    Rt.advance(K0 + 5, NTR - 5, TPUR, H)
    assert_same(sa, jw.snap(twin, Rt), 'the clone made mid-rollout against the uncut run')
    # the model matters: without it the same ticks end elsewhere
    ge, Re = jw.fresh()
    Re.set_joints(None)
    Re.advance(K0, NTR, TPUR, H)
    assert np.abs(Re.state()[0] - sa['q']).max() > 1e-6
    # the gait entry once: one call against one call per tick
    gf, Rf = jw.fresh(tick_log=NTR, step_log=n_upd)
    gait_f = host.BatchGaitOptimizer(gf)
    Rf.advance(K0, NTR, TPUR, H, gait=gait_f, gait_opt_freq=3)
    gh, Rh = jw.fresh(tick_log=NTR, step_log=n_upd)
    gait_h = host.BatchGaitOptimizer(gh)
    for k in range(K0, K0 + NTR):
        Rh.advance(k, 1, TPUR, H, gait=gait_h, gait_opt_freq=3)
    sf = jw.snap(gf, Rf)
    assert_same(sf, jw.snap(gh, Rh), 'the gait entry: one call per tick against one call')
    same_bytes(Rh.tick_log(), Rf.tick_log(), 'the gait entry: tick log')
    same_bytes(gh.step_log(), gf.step_log(), 'the gait entry: step log')
    assert np.all(sf['jrec'][:, 0] == NTR * SUBR)
    gait_f.close(); gait_h.close()


# ---- 6. physics that a wrong sign or a wrong row would break ----
def test_a_large_armature_takes_the_joints_torque(world):
    """I_a = 1e4 on one joint, the feet held with none in contact, the robot at rest in free fall, a torque on that joint alone: its acceleration is
    t / I_a to within I_link / I_a = M_jj / I_a, which the restatement supplies; asserted with a factor 10 over that ratio, and against the
    restatement within 1e-9"""
    cfg = world.cfg
    g, R, models, _ = bare_plant(cfg)
    ia, t = 1e4, 30.0
    q = np.tile(np.array(cfg['init_config'], float), (B, 1))
    joints = [2, 5, 6, 10]
    J, tau = jk.transparent(B), np.zeros((B, 12))
    for b, j in enumerate(joints):
        J[b, j, jk.JIA] = ia
        tau[b, j] = t if b % 2 == 0 else -t
    R.set_joints(J, (100.0, 1.0))
    sol, st = R.forward_dynamics(q, np.zeros((B, 18)), tau, np.zeros((B, 4), np.int32))
    assert np.all(st == 0)
    for b, j in enumerate(joints):
        M, _, _ = models[b].robot.dynamics_terms(q[b], np.zeros(18))
        ratio = M[6 + j, 6 + j] / ia
        want, _, _ = jk.dynamics(jk.HELD, models[b], J[b], q[b], np.zeros(18), tau[b], np.zeros(4, int))
        a = sol[b, 6 + j]
        print('instance %d joint %d: a %.6g, t / I_a %.6g, relative difference %.3g, I_link / I_a %.3g' % (b, j, a, tau[b, j] / ia, abs(a * ia / tau[b, j] - 1), ratio))
        assert abs(a * ia / tau[b, j] - 1) <= 10 * ratio and ratio < 1e-4, (b, j)
        assert np.abs(sol[b] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (b, j)


def test_the_limp_robot_drops_onto_its_stops_as_the_restatement_does(world):
    """wb_joint_plant_kit's limp drop through srbm_wb_ground_step_dev: a zero control action, the A1 ranges, one instance, DROP_TICKS ticks of 1 ms at
    S = 4.  Over the first DROP_CHECK_TICKS ticks (q, v, js) within 1e-9 of the restatement, the contact flags equal and the anchors within 1e-9;
    at the end the largest excursion beyond a range and |v|_inf within 2 x the constants recorded from the restatement, all four calves on their
    stops, every foot on the ground"""
    cfg = world.cfg
    c = jk.drop_case(cfg)
    g = host.BatchMPC(cfg, 1)
    R = ControllerRollout(g)
    R.set_plant(PLANT_TORQUE_DRIVEN, np.zeros(12), np.zeros(12), c['lim'], jk.DROP_S)
    R.set_ground(c['ground'])
    R.set_joints(c['joints'], c['stops'])
    want = jk.drop_restated(cfg, ticks=jk.DROP_CHECK_TICKS)
    d = dict(q=Dev(c['q'][None]), v=Dev(c['v'][None]), cs=Dev(np.zeros((1, 4, 3))), ctl=Dev(c['control'][None]), st=Dev(np.array([[2, 8]], np.int32)))
    worst = 0.0
    for k in range(jk.DROP_TICKS):
        R.ground_step_dev(k, jk.DROP_H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value)
        if k < jk.DROP_CHECK_TICKS:
            g.synchronize()
            qn, vn, csn, jsn = want['first'][k]
            errs = [np.abs(d['q'].get()[0] - qn).max(), np.abs(d['v'].get()[0] - vn).max(), np.abs(R.joint_state()[0] - jsn).max()]
            cs_error(d['cs'].get()[0], csn, 'tick %d' % k)
            worst = max(worst, max(errs))
            assert max(errs) <= 1e-9, (k, errs)
    g.synchronize()
    q, v, cs, jrec = d['q'].get()[0], d['v'].get()[0], d['cs'].get()[0], R.joint_record()[0]
    assert jrec[0] == jk.DROP_TICKS * jk.DROP_S
    print('limp drop on the device: worst error over the first %d ticks %.3g; at the end |v|_inf %.4g (recorded %.4g), largest excursion %.4g rad (recorded %.4g), mask %d' % (
        jk.DROP_CHECK_TICKS, worst, np.abs(v).max(), jk.DROP_V_END, jrec[2], jk.DROP_EXCURSION, int(jrec[5])))
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(v))
    assert 0 < jrec[2] <= 2 * jk.DROP_EXCURSION and np.abs(v).max() <= 2 * jk.DROP_V_END
    assert int(jrec[5]) == 0b100100100100 and np.all(cs[:, 0] == 1) and jrec[1] > 0
    assert np.any(want['first'][-1][2][:, 0] == 1)          # the feet touched down within the ticks that were compared
