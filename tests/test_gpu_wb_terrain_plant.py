"""The terrain of the torque-driven plant's ground on the GPU (srbm_wb_plant_set_terrain; csrc/srbm_wb_terrain.hiph through
bilevel-gait-gen_amd/controller_rollout.py) against the numpy restatement of tests/wb_terrain_plant_kit.py: one unbounded level patch is the flat
ground bit for bit; the law and the solve alone; the step alone; the rollout three ways bit for bit with every record the read-back of its tick and
its tick summaries folded on the device; the setting leaves no trace; physics on a slope; the refusals and the clone.  The world is
test_gpu_controller_rollout.py's: 4 Config-B instances after one cold start, ticks of 10 ms, an MPC update every 5 ticks, instance 2 pushed in
tick 3.  Every test sets a terrain."""
import numpy as np
import pytest

import controller_rollout_kit as kit
import tick_summary_kit as tsk
import wb_ground_plant_kit as gk
import wb_terrain_plant_kit as tk
import wb_torque_plant_kit as fd
from gpu_kit import same_bytes
from srbm_loader import host, tick_summary as ts
from srbm_loader.controller_rollout import (ControllerRollout, TICK_LOG_FIELDS, GROUND_PLANT_LOG_FIELDS, GROUND_WORD_OFFSET, decode_ground_word, terrain_patch,
                                            FLAG_PUSH, FLAG_UPDATE, FLAG_BREAKDOWN, PLANT_QP_ACCELERATION, PLANT_TORQUE_DRIVEN)
from test_gpu_controller_rollout import World, Dev, assert_same
from test_gpu_wb_ground_plant import own_bodies, cs_error, Rollouts, run_ground_chain, ground_snapshot

pytestmark = pytest.mark.gpu
B, H, TPU = kit.B, kit.TICK_DT, kit.TPU
F = dict(TICK_LOG_FIELDS, **GROUND_PLANT_LOG_FIELDS)
NT = 10                 # ticks of the rollouts: the push in tick 3 and the MPC update after tick 5 are inside
SUB = 4                 # their sub-steps per tick


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def rollouts(world):
    return Rollouts(world)


def step_on_device(g, R, c, pushed):
    g.plant_set_push(c['push_time'], c['impulse']) if pushed else g.plant_set_push()
    d = dict(q=Dev(c['q']), v=Dev(c['v']), cs=Dev(c['cs']), ctl=Dev(c['control']), st=Dev(c['status']), sol=Dev(np.zeros((B, 30))))
    R.ground_step_dev(c['k'], H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value, d['sol'].p.value)
    g.synchronize()
    return d['q'].get(), d['v'].get(), d['sol'].get(), d['cs'].get()


# ---- 1. level terrain is the ground, bit for bit ----
def test_one_unbounded_level_patch_is_the_flat_ground_bit_for_bit(world, rollouts):
    """one unbounded level patch per instance with the ground's z0 and mu, through the terrain kernels, against the flat ground on the same inputs:
    srbm_wb_ground_dynamics on the ground's solve cases (sol, cs, status), srbm_wb_ground_step_dev on its step cases at S = 1 and 3 with and without
    pushes (q, v, cs, sol), and a logged advance of NT ticks on the ground test's rollout ground (plant, cs, trajectories, q_des, tick log, step log)"""
    cfg = world.cfg
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    lists, models = own_bodies(cfg)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    kp, kd, lim = fd.step_actuators(cfg)
    R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 1)
    for c, case in enumerate(gk.solve_cases(cfg, models)):
        R.set_ground(case['ground']); R.set_terrain(None)
        flat = R.ground_dynamics(case['q'], case['v'], case['tau'], case['cs'])
        R.set_terrain(tk.level_terrain(case['ground']))
        level = R.ground_dynamics(case['q'], case['v'], case['tau'], case['cs'])
        for a, b, name in zip(flat, level, ('(a, F)', 'cs', 'status')):
            same_bytes(b, a, 'solve call %d: %s' % (c, name))
        assert np.abs(flat[0][:, 18:]).max() > 1.0
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        for rnd, c in enumerate(gk.step_cases(cfg, models, H)):
            R.set_ground(c['ground'])
            for pushed in (False, True):
                R.set_terrain(None)
                flat = step_on_device(g, R, c, pushed)
                R.set_terrain(tk.level_terrain(c['ground']))
                level = step_on_device(g, R, c, pushed)
                for a, b, name in zip(flat, level, ('q+', 'v+', '(a, F)', 'cs+')):
                    same_bytes(b, a, 'S %d round %d pushed %s: %s' % (S, rnd, pushed, name))
    w, ro = world, rollouts
    ga, Ra = ro.fresh(tick_log=NT, step_log=4)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = ro.fresh(tick_log=NT, step_log=4)
    Rb.set_terrain(tk.level_terrain(ro.ground))
    Rb.advance(0, NT, TPU, H)
    assert_same(ground_snapshot(w, ga, Ra, NT), ground_snapshot(w, gb, Rb, NT), 'the rollout on the level terrain against the flat ground')
    same_bytes(Rb.tick_log(), Ra.tick_log(), 'tick log')
    same_bytes(gb.step_log(), ga.step_log(), 'step log')
    assert decode_ground_word(Ra.tick_log()[:, :, 63])['in_contact'].any()


# ---- 2. the law and the solve alone ----
def test_the_law_and_the_solve_alone_against_the_restatement(world):
    """srbm_wb_ground_dynamics with a terrain on kit.solve_cases: 3 to 4 patches per instance with planes and frictions of their own, the four feet
    of an instance on different patches in different branches -- stick, slip and clamp on a first touch and with an old anchor, a stored patch that
    is another one, a foot over no patch, a foot under an overlaid patch, an empty patch.  (a, F) within 1e-9 max(1, |x|_inf), the flags of cs_out
    (the patch number) equal and its anchors within 1e-9, the dynamics residual within 1e-9 max(1, |tau|_inf), N >= 0, zero force in the air; the
    device-pointer entry returns the same bytes; a NaN configuration gives status 1 and zeros"""
    cfg = world.cfg
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    lists, models = own_bodies(cfg)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    R.set_plant(PLANT_TORQUE_DRIVEN, *fd.step_actuators(cfg), 1)
    cases = tk.solve_cases(cfg, models)
    worst_x = worst_r = worst_c = 0.0
    for c, case in enumerate(cases):
        R.set_ground(case['ground']); R.set_terrain(case['terrain'])
        sol, cs_out, st = R.ground_dynamics(case['q'], case['v'], case['tau'], case['cs'])
        assert np.all(st == 0), (c, st)
        for b in range(B):
            where = 'call %d instance %d' % (c, b)
            want, cs_want, infos = tk.terrain_dynamics(models[b], case['q'][b], case['v'][b], case['tau'][b], case['cs'][b], case['ground'][b], case['terrain'][b])
            assert [(i['branch'], i['first'], i['patch']) for i in infos] == case['want'][b], where
            ex = np.abs(sol[b] - want).max() / max(1.0, np.abs(want).max())
            ec = cs_error(cs_out[b], cs_want, where)
            res = kit.dynamics_residual(models[b], case['q'][b], case['v'][b], sol[b, :18], case['tau'][b], sol[b, 18:].reshape(4, 3), np.ones(4, int))
            er = np.abs(res).max() / max(1.0, np.abs(case['tau'][b]).max())
            worst_x, worst_r, worst_c = max(worst_x, ex), max(worst_r, er), max(worst_c, ec)
            print('%s %s: (a, F) %.3g relative, anchors %.3g, dynamics residual %.3g relative' % (where, [i['branch'] for i in infos], ex, ec, er))
            assert ex <= 1e-9 and er <= 1e-9, where
            for i in range(4):
                Fi = sol[b, 18 + 3 * i:21 + 3 * i]
                if infos[i]['branch'] == tk.AIR:
                    assert np.all(Fi == 0) and np.all(cs_out[b, i] == 0), where
                else:
                    assert Fi @ infos[i]['n'] >= -1e-9 * max(1.0, np.abs(Fi).max()) and cs_out[b, i, 0] == 1 + infos[i]['patch'], where
    print('worst over all cases: (a, F) %.3g relative, anchors %.3g, dynamics residual %.3g relative' % (worst_x, worst_c, worst_r))
    case = cases[1]
    R.set_ground(case['ground']); R.set_terrain(case['terrain'])
    d = dict(q=Dev(case['q']), v=Dev(case['v']), tau=Dev(case['tau']), cs=Dev(case['cs']), sol=Dev(np.zeros((B, 30))), out=Dev(np.zeros((B, 4, 3))),
             st=Dev(np.full(B, -1, np.int32)))
    R.ground_dynamics_dev(d['q'].p.value, d['v'].p.value, d['tau'].p.value, d['cs'].p.value, d['sol'].p.value, d['out'].p.value, d['st'].p.value)
    g.synchronize()
    sol, cs_out, st = R.ground_dynamics(case['q'], case['v'], case['tau'], case['cs'])
    same_bytes(d['sol'].get(), sol, 'the device-pointer entry against the host entry: (a, F)')
    same_bytes(d['out'].get(), cs_out, 'the device-pointer entry against the host entry: cs')
    assert np.array_equal(d['st'].get(), st)
    qn = case['q'].copy(); qn[2, 9] = np.nan
    sol, cs_out, st = R.ground_dynamics(qn, case['v'], case['tau'], case['cs'])
    assert st.tolist() == [0, 0, 1, 0] and np.all(sol[2] == 0) and np.all(np.isfinite(sol))


# ---- 3. the step alone ----
def test_the_terrain_step_alone_against_the_restatement(world):
    """srbm_wb_ground_step_dev with a terrain on kit.step_cases at S = 1 and 3: in sub-step 2 a foot touches down on a slope, a foot lifts off and a
    foot slides from one patch onto another (re-anchored there); a joint in its limit, zero control actions, pushes.  q+, v+ and (a, F) of the last
    sub-step within 1e-9, the flags of cs+ equal and its anchors within 1e-9, push decisions exact"""
    cfg = world.cfg
    ctrl = kit.Model(cfg)
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    lists, models = own_bodies(cfg)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    kp, kd, lim = fd.step_actuators(cfg)
    touched = lifted = slid = False
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        for rnd, c in enumerate(tk.step_cases(cfg, models, H)):
            R.set_ground(c['ground']); R.set_terrain(c['terrain'])
            off = (c['status'][:, 1] & 255) > 1
            res = {pushed: step_on_device(g, R, c, pushed) for pushed in (False, True)}
            for b in range(B):
                where = 'S %d round %d instance %d' % (S, rnd, b)
                assert (not np.array_equal(res[True][1][b], res[False][1][b])) == bool(c['want_push'][b]), where
                same_bytes(res[True][2][b], res[False][2][b], where + ': (a, F) does not see the push')
                for pushed in (False, True):
                    push = (c['push_time'][b], c['impulse'][b]) if pushed else None
                    qn, vn, csn, info = tk.terrain_step(models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], c['ground'][b],
                                                        c['terrain'][b], H, S, c['k'], ctrl.mass, ctrl.Ir_inv, push)
                    assert info['pushed'] == (pushed and bool(c['want_push'][b])), where
                    eq, ev = np.abs(res[pushed][0][b] - qn).max(), np.abs(res[pushed][1][b] - vn).max()
                    es = np.abs(res[pushed][2][b] - info['sol']).max() / max(1.0, np.abs(info['sol']).max())
                    ec = cs_error(res[pushed][3][b], csn, where)
                    print('%s pushed %s: q+ %.3g v+ %.3g (a, F) %.3g relative, anchors %.3g' % (where, pushed, eq, ev, es, ec))
                    assert eq <= 1e-9 and ev <= 1e-9 and es <= 1e-9, (where, pushed, eq, ev, es)
            if S == 3:
                cs1 = res[False][3]
                touched |= bool(cs1[tk.TOUCH_DOWN[0], tk.TOUCH_DOWN[1], 0] == 1 + tk.TOUCH_DOWN[1] and c['cs'][tk.TOUCH_DOWN[0], tk.TOUCH_DOWN[1], 0] == 0)
                lifted |= bool(cs1[tk.LIFT_OFF[0], tk.LIFT_OFF[1], 0] == 0)
                slid |= bool(cs1[tk.SLIDE[0], tk.SLIDE[1], 0] == 5 and c['cs'][tk.SLIDE[0], tk.SLIDE[1], 0] == 1 + tk.SLIDE[1])
    assert touched and lifted and slid
    assert R.tick_log_count() == 0


# ---- 4. the rollout ----
def terrain_fresh(ro, terrain, **kw):
    g, R = ro.fresh(**kw)
    R.set_ground(tk.rollout_ground())
    R.set_terrain(terrain)
    return g, R


def test_the_rollout_three_ways_bitwise_every_record_the_read_back_of_its_tick_and_its_summaries(world, rollouts):
    """on a base slope with a low-friction patch under the two left feet: the plant, cs, the trajectories, q_des, the tick log and the step log of NT
    ticks in one call, one call per tick and as the host-driven chain; every record's fields 58..63 against the restated tick on the chain's control
    (the clamped count and the word exact, the rest within 1e-9 relative, field 60 the smallest NORMAL force over the planned feet); a slip bit and
    a plan-against-ground bit are seen; the tick summaries folded on the device equal tick_summary_kit's fold byte for byte"""
    w, ro = world, rollouts
    terrain = tk.rollout_terrain(w.q, w.model.legs)
    gr = tk.rollout_ground()
    ga, Ra = terrain_fresh(ro, terrain, tick_log=NT, step_log=4)
    Ra.advance(0, NT, TPU, H)
    gb, Rb = terrain_fresh(ro, terrain, tick_log=NT, step_log=4)
    for k in range(NT):
        Rb.advance(k, 1, TPU, H)
    gc, Rc = terrain_fresh(ro, terrain, step_log=4)
    chain = run_ground_chain(gc, Rc, w.q, w.v, np.zeros((B, 4, 3)), 0, NT, TPU)
    sa = ground_snapshot(w, ga, Ra, NT)
    for name, g, R in (('one call per tick', gb, Rb), ('host-driven chain', gc, Rc)):
        assert_same(sa, ground_snapshot(w, g, R, NT), name)
    assert Ra.tick_log_count() == Rb.tick_log_count() == NT and Rc.tick_log_count() == 0
    log = Ra.tick_log()
    same_bytes(log, Rb.tick_log(), 'tick log: one call against one per tick')
    same_bytes(ga.step_log(), gb.step_log(), 'step log: one call against one per tick')
    same_bytes(ga.step_log(), gc.step_log(), 'step log: one call against the chain')
    same_bytes(chain[-1]['cs_next'], sa['cs'], 'cs after the last tick')
    kp, kd, lim = ro.act
    in_contact = slipped = differed = 0
    for k, c in enumerate(chain):
        r = log[k]
        where = 'tick %d' % k
        assert np.all(r[:, F['tick']] == k) and np.all(r[:, F['plant_kind']] == 1), where
        same_bytes(r[:, F['torques']], c['control'][:, 24:], where + ': torques')
        flags = r[:, F['flags']].astype(int)
        assert np.array_equal(flags & FLAG_PUSH != 0, np.array([b == kit.PUSHED and k == kit.PUSH_TICK for b in range(B)])), where
        assert np.all((flags & FLAG_UPDATE != 0) == (k > 0 and k % TPU == 0)) and np.all(flags & FLAG_BREAKDOWN == 0), where
        qp_forces = np.array([kit.unstack_forces(c['qp_sol'][b], c['contact'][b]).reshape(12) for b in range(B)])
        word = decode_ground_word(r[:, F['ground_word']])
        assert np.all(word['ground']), where
        assert np.array_equal(word['in_contact'], c['cs_next'][:, :, 0] != 0), where
        for b in range(B):
            off = (c['status'][b, 1] & 255) > 1
            qn, vn, csn, info = tk.terrain_step(ro.models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off, kp[b], kd[b], lim[b], gr, terrain[b], H, SUB, k,
                                                w.model.mass, w.model.Ir_inv, (w.push_time[b], w.impulse[b]))
            sol = info['sol']
            N = np.array([i['N'] for i in info['infos']])
            held = c['contact'][b] != 0
            want = (info['clamped'], info['deviation'], N[held].min() if held.any() else 0.0, np.abs(sol[:18] - c['qp_sol'][b, :18]).max(),
                    np.abs(sol[18:] - qp_forces[b]).max())
            got = r[b, 58:63]
            assert got[0] == want[0], (where, b, got[0], want[0])
            for i in range(1, 5):
                assert abs(got[i] - want[i]) <= 1e-9 * max(1.0, abs(want[i])), (where, b, i, got[i], want[i])
            assert got[2] >= 0, (where, b)
            assert r[b, 63] == GROUND_WORD_OFFSET + gk.ground_word(csn, info['infos'], c['contact'][b]), (where, b)
            es = np.abs(c['sol'][b] - sol).max() / max(1.0, np.abs(sol).max())
            eq = max(np.abs(chain[k + 1]['q'][b] - qn).max(), np.abs(chain[k + 1]['v'][b] - vn).max()) if k + 1 < NT else 0.0
            assert es <= 1e-9 and eq <= 1e-9, (where, b, es, eq)
            cs_error(c['cs_next'][b], csn, (where, b))
        in_contact += int(word['in_contact'].sum()); slipped += int(word['slipping'].sum()); differed += int(word['plan_differs'].sum())
    patches = sorted(set(np.concatenate([c['cs_next'][:, :, 0].ravel() for c in chain]).tolist()))
    print('feet in contact %d, slipping %d, off the plan %d over %d ticks x %d instances; in_contact values seen %s' % (in_contact, slipped, differed, NT, B, patches))
    assert slipped >= 1 and differed >= 1 and 1.0 in patches and 2.0 in patches
    # the tick summaries of that rollout, folded on the device
    ref = ts.reference_from_config(w.cfg, B)
    r2, dz, tilt, v2 = tsk.criteria_of_log(log, ref)
    crit = ts.criteria(z_min=0.2, tilt_max=0.5, r2_settle=r2, dz_settle=dz, tilt_settle=tilt, v2_settle=v2)
    ts.enable(ga, crit, ref)
    ts.fold(ga)
    want = tsk.fold(log, crit, ref)
    same_bytes(ts.summaries(ga), want, 'tick summaries: the device fold against the restatement')
    S = ts.SUMMARY_FIELDS
    assert (want[:, S['ground_records']] == NT).all() and want[:, S['slip_sum']].sum() == slipped and want[:, S['plan_mismatch_sum']].sum() == differed


# ---- 5. no trace ----
def test_a_terrain_removed_without_a_ground_or_under_kind_0_leaves_no_trace(world, rollouts):
    w, ro, n = world, rollouts, 6
    terrain = tk.rollout_terrain(w.q, w.model.legs)

    def compare(a, b, what):
        (ga, Ra), (gb, Rb) = a, b
        Ra.advance(0, n, TPU, H); Rb.advance(0, n, TPU, H)
        assert_same(ground_snapshot(w, ga, Ra, n), ground_snapshot(w, gb, Rb, n), what)
        same_bytes(Ra.tick_log(), Rb.tick_log(), what + ': tick log')
        same_bytes(ga.step_log(), gb.step_log(), what + ': step log')
        return Ra.tick_log()
    a = ro.fresh(tick_log=n, step_log=2)
    a[1].set_terrain(terrain); a[1].set_terrain(None)
    la = compare(a, ro.fresh(tick_log=n, step_log=2), 'a terrain set and removed against the ground that never had one')
    assert np.all(la[:, :, 63] >= GROUND_WORD_OFFSET)
    a = ro.fresh(tick_log=n, step_log=2)
    a[1].set_terrain(terrain); a[1].set_ground(None)
    la = compare(a, ro.fresh(ground=False, tick_log=n, step_log=2), 'a terrain whose ground was removed against kind 1 with the feet held')
    assert np.all(la[:, :, 57] == 1) and np.all(la[:, :, 63] == 0) and np.all(a[1].contact_state() == 0)
    a = w.fresh(tick_log=n, step_log=2)
    a[1].set_plant(PLANT_QP_ACCELERATION, *ro.act, SUB)
    a[1].set_ground(ro.ground); a[1].set_terrain(terrain)
    la = compare(a, w.fresh(tick_log=n, step_log=2), 'kind 0 with a ground and a terrain against kind 0')
    assert np.all(la[:, :, 57:] == 0)


# ---- 6. physics on a slope ----
def test_on_a_slope_the_robot_rests_above_the_friction_angle_and_slides_below_it_by_the_closed_form(world):
    """the kit's slope case through srbm_wb_ground_step_dev, constant control, no MPC, instances 0 and 2 with mu well above tan(theta), 1 and 3
    below: (a) |v|_inf < V_REST and |sum N - m g cos(theta)| / (m g) < W_REST; (b) all four feet slipping (|T| = mu N) and the base's downhill
    acceleration over the last 100 ticks within the kit's band of g (sin(theta) - mu cos(theta))"""
    cfg = world.cfg
    c = tk.slope_case(cfg)
    idx = [0, 1, 0, 1]
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    R.set_plant(PLANT_TORQUE_DRIVEN, c['kp'], c['kd'], c['lim'], gk.SETTLE_S)
    R.set_plant_bodies(*fd.bodies_arrays([c['bodies']] * B))
    R.set_ground(c['ground'])
    R.set_terrain(c['terrain'][idx])
    d = dict(q=Dev(np.tile(c['q'], (B, 1))), v=Dev(np.zeros((B, 18))), cs=Dev(np.zeros((B, 4, 3))), ctl=Dev(np.tile(c['control'], (B, 1))),
             st=Dev(np.zeros((B, 2), np.int32)), sol=Dev(np.zeros((B, 30))))
    marks = []
    for k in range(gk.SETTLE_TICKS):
        R.ground_step_dev(k, gk.SETTLE_H, d['q'].p.value, d['v'].p.value, d['cs'].p.value, d['ctl'].p.value, d['st'].p.value, d['sol'].p.value)
        if k + 1 in tk.SLOPE_MARKS:
            g.synchronize()
            marks.append(d['q'].get())
    g.synchronize()
    q, v, sol, cs = d['q'].get(), d['v'].get(), d['sol'].get(), d['cs'].get()
    assert np.all(np.isfinite(q)) and np.all(cs[:, :, 0] == 1)
    want = tk.slide_closed_form()
    for b in range(B):
        vmax, werr, acc = tk.slope_measures(v[b], sol[b], [m[b] for m in marks], c)
        Fb = sol[b, 18:].reshape(4, 3)
        N = Fb @ c['n']
        T = np.linalg.norm(Fb - N[:, None] * c['n'][None, :], axis=1)
        if idx[b] == 0:
            print('instance %d (a): |v|_inf %.3g (V_REST %g), normal-force error %.3g (W_REST %g)' % (b, vmax, gk.V_REST, werr, gk.W_REST))
            assert vmax < gk.V_REST and werr < gk.W_REST, b
            assert np.all(T < tk.SLOPE_MU_REST * N), b
        else:
            print('instance %d (b): downhill acceleration %.5f against %.5f, deviation %.3g (band %g)' % (b, acc, want, abs(acc - want), tk.SLOPE_SLIDE_BAND))
            assert np.all(N > 0) and np.all(np.abs(T - tk.SLOPE_MU_SLIDE * N) <= 1e-9 * np.maximum(1.0, N)), (b, T, N)
            assert abs(acc - want) <= tk.SLOPE_SLIDE_BAND, b
    same_bytes(q[:2], q[2:], 'the two copies of the cases')


# ---- 7. refusals and the clone ----
def test_refusals_leave_everything_untouched_and_a_clone_made_mid_rollout_ends_where_the_original_ends(world, rollouts):
    w, ro = world, rollouts
    terrain = tk.rollout_terrain(w.q, w.model.legs)
    g, R = terrain_fresh(ro, terrain, tick_log=8, step_log=1)
    R.advance(0, 3, TPU, H)
    g.synchronize()
    twin = g.clone()                        # mid-rollout: the terrain goes along with the ground and the contact state
    Rt = ControllerRollout(twin)
    same_bytes(Rt.contact_state(), R.contact_state(), 'cs of the clone')
    assert R.contact_state()[:, :, 0].any()

    def state():
        return ground_snapshot(w, g, R, 3), (R.tick_log_count(), g.step_log_count())
    s0, c0 = state()

    def changed(idx, value):
        a = terrain.copy(); a[idx] = value
        return a
    cases = [(changed((2, 1, 0), np.nan), 'instance 2, patch 1, field 0'), (changed((0, 0, 3), np.nan), 'instance 0, patch 0, field 3'),
             (changed((1, 0, 4), np.inf), 'instance 1, patch 0, field 4'), (changed((3, 1, 4), np.nan), 'instance 3, patch 1, field 4'),
             (changed((0, 1, 5), -np.inf), 'instance 0, patch 1, field 5'), (changed((2, 0, 6), np.nan), 'instance 2, patch 0, field 6'),
             (changed((1, 1, 7), np.inf), 'instance 1, patch 1, field 7'), (changed((3, 0, 7), -0.1), 'instance 3, patch 0, field 7'),
             (np.tile(tk.patch(), (B, 9, 1)), 'n_patches 9'), (np.zeros((B, 0, 8)), 'n_patches 0')]
    for bad, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            R.set_terrain(bad)
        s1, c1 = state()
        assert c1 == c0, msg
        assert_same(s0, s1, 'after the refused call (%s)' % msg)
    # the contact state: 0 .. n_patches while a terrain is set, 0 or 1 without one
    cs = R.contact_state()
    for value in (3.0, 1.5, -1.0):
        bad_cs = cs.copy(); bad_cs[1, 2, 0] = value
        with pytest.raises(RuntimeError, match='instance 1, foot 2'):
            R.set_contact_state(bad_cs)
    assert_same(s0, state()[0], 'after the refused contact states')
    two = np.zeros_like(cs); two[1, 2, 0] = 2.0
    R.set_contact_state(two)
    R.set_contact_state(cs)
    R.set_terrain(None)
    with pytest.raises(RuntimeError, match='instance 1, foot 2'):
        R.set_contact_state(two)
    R.set_terrain(terrain)
    assert_same(s0, state()[0], 'after the terrain was removed and set again')
    R.advance(3, 4, TPU, H)
    Rt.advance(3, 4, TPU, H)
    assert_same(ground_snapshot(w, g, R, 7), ground_snapshot(w, twin, Rt, 7), 'the original against the clone made mid-rollout')
    assert R.tick_log_count() == 7 and Rt.tick_log_count() == 0
    assert np.all(R.tick_log()[:, :, F['ground_word']] >= GROUND_WORD_OFFSET) and (R.contact_state()[:, :, 0] == 2).any()
    # a terrain needs a ground; bounds may be infinite, a reversed pair is an empty patch
    c, Rc = w.fresh()
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_ground'):
        Rc.set_terrain(terrain)
    Rc.set_ground(ro.ground)
    Rc.set_terrain([terrain_patch(), terrain_patch(x=(1.0, 0.0), y=(-np.inf, np.inf), mu=0.0)])
    with pytest.raises(ValueError):
        Rc.set_terrain(np.zeros((B, 2, 7)))
