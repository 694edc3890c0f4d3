"""Whole-controller rollouts on the GPU (srbm_controller_advance, srbm_wb_plant_*, srbm_tick_log_*; csrc/srbm_wb_plant.hiph through
bilevel-gait-gen_amd/controller_rollout.py): the entry in one call, tick by tick and as a host-driven chain of the three device entries, bit for bit;
the tick log as the read-back of every tick; the plant step alone and the whole loop against the numpy restatement of
tests/controller_rollout_kit.py; the plant as the whole-body dynamics; the update period, the summaries, the refusals and the clone.
4 Config-B instances (N = 20, dt = 0.05) after one cold start, ticks of 10 ms (35 of them cross the first contact switch at 0.3 s), an MPC update
every 5 ticks, instance 2 pushed in tick 3.  Every test works on clones of that batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import controller_rollout_kit as kit
from gpu_kit import same_bytes
from srbm_loader import host
from srbm_loader import rollout_summary as rs
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import ControllerRollout, TICK_LOG_FIELDS as F, FLAG_PUSH, FLAG_UPDATE, FLAG_COAST
from srbm_loader.workloads import config_b_instance, instances

pytestmark = pytest.mark.gpu
B, H, TPU = kit.B, kit.TICK_DT, kit.TPU
hip = None


class Dev:
    """a device array (hipMalloc through the HIP runtime, as test_gpu_control_tick.py has it)"""

    def __init__(self, a):
        global hip
        hip = hip or C.CDLL('libamdhip64.so')
        self.a = np.ascontiguousarray(a); self.p = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(self.a.nbytes)) == 0
        self.put(self.a)

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=self.a.dtype)
        assert a.nbytes == self.a.nbytes
        assert hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice (synchronous)

    def get(self):
        out = np.empty_like(self.a)
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.a.nbytes), 2) == 0
        return out

    def __del__(self):
        hip.hipFree(self.p)


class World:
    """the cold-started batch, the plant's first (q, v), the pushes; and, computed once on first use and never modified, the 35 ticks as a
    host-driven chain (every output of every tick) and as one logged call"""

    def __init__(self):
        self.cfg = host.load_config('a1_configuration')
        self.model = kit.Model(self.cfg)
        self.states, self.ees = instances(self.cfg, config_b_instance, B)
        self.base = host.BatchMPC.cold_start(self.cfg, self.states, self.ees)
        assert self.base.get_trajectory(0, 1)[0].init_time == 0.0
        self.q0 = np.tile(np.array(self.cfg['init_config'], float), (B, 1))
        qd, vd, _, st = self.base.clone().get_targets_from_traj(0.0, self.q0)
        assert np.all(st == 0)
        self.q, self.v = kit.first_measured(qd, vd)
        self.push_time, self.impulse = kit.pushes()
        self._chain = self._logged = None

    def fresh(self, tick_log=0, step_log=0, base=None, q=None, v=None, push=True):
        g = (base or self.base).clone()
        R = ControllerRollout(g)
        R.reset(self.q0[:g.batch])
        R.set_state(self.q if q is None else q, self.v if v is None else v)
        if push:
            g.plant_set_push(self.push_time[:g.batch], self.impulse[:g.batch])
        if tick_log:
            R.tick_log_enable(tick_log)
        if step_log:
            g.step_log_enable(step_log)
        return g, R

    @property
    def chain(self):
        if self._chain is None:
            g, R = self.fresh(step_log=8)
            self._chain = run_chain(g, R, self.q, self.v, 0, kit.NTICKS, TPU)
            self._chain_end = snapshot(self, g, R, kit.NTICKS)
        return self._chain

    @property
    def logged(self):
        if self._logged is None:
            g, R = self.fresh(tick_log=kit.NTICKS, step_log=8)
            R.advance(0, kit.NTICKS, TPU, H)
            self._logged = R.tick_log()
            self._logged_end = snapshot(self, g, R, kit.NTICKS)
        return self._logged


@pytest.fixture(scope='module')
def world():
    return World()


def run_chain(g, R, q, v, first, ticks, tpu, h=H):
    """the loop driven from the host on the caller's device arrays: srbm_control_tick_dev, srbm_wb_plant_step_dev, srbm_get_real_time_update_dev.
    -> one dict per tick: the measured (q, v) and every output of the tick"""
    T = ControlTick(g)
    n = g.batch
    d = dict(q=Dev(q), v=Dev(v), t=Dev(np.zeros(n)), control=Dev(np.zeros((n, 36))), qp_sol=Dev(np.zeros((n, 30))), status=Dev(np.zeros((n, 2), np.int32)),
             contact=Dev(np.zeros((n, 4), np.int32)), state=Dev(np.zeros((n, 13))), ee=Dev(np.zeros((n, 4, 3))))
    out = []
    for k in range(first, first + ticks):
        g.synchronize()
        d['t'].put(np.full(n, k * h))
        rec = dict(q=d['q'].get(), v=d['v'].get())
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        g.synchronize()
        rec.update({key: d[key].get() for key in ('control', 'qp_sol', 'status', 'contact', 'state', 'ee')})
        R.plant_step_dev(k, h, d['q'].p.value, d['v'].p.value, d['qp_sol'].p.value, d['status'].p.value)
        if k > 0 and k % tpu == 0:
            g.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
        out.append(rec)
    g.synchronize()
    R.set_state(d['q'].get(), d['v'].get())          # the batch's own plant state is what the chain ended with (for snapshot)
    return out


def snapshot(w, g, R, next_tick):
    """what a rollout leaves behind: the plant state, the trajectories, and the batch's q_des seen through the targets of one more tick on a clone
    (q_des is the IK guess of that tick)"""
    q, v = R.state()
    c = g.clone()
    probe = ControlTick(c).tick(q, v, next_tick * H)
    return dict(q=q, v=v, trajectory=np.frombuffer(bytes(g.get_trajectory()), np.uint8), q_des=probe['q_des'], probe_sol=probe['qp_sol'])


def assert_same(a, b, what):
    for k in a:
        same_bytes(a[k], b[k], '%s: %s' % (what, k))


def test_one_call_twelve_calls_and_the_host_driven_chain_bitwise(world):
    w, n = world, 12
    ga, Ra = w.fresh(tick_log=n, step_log=4)
    Ra.advance(0, n, TPU, H)
    gb, Rb = w.fresh(tick_log=n, step_log=4)
    for k in range(n):
        Rb.advance(k, 1, TPU, H)
    gc, Rc = w.fresh(step_log=4)
    run_chain(gc, Rc, w.q, w.v, 0, n, TPU)
    gd, Rd = w.fresh()
    Rd.advance(0, n, TPU, H)
    sa = snapshot(w, ga, Ra, n)
    for name, g, R in (('twelve calls', gb, Rb), ('host-driven chain', gc, Rc), ('no logs', gd, Rd)):
        assert_same(sa, snapshot(w, g, R, n), name)
    assert Ra.tick_log_count() == Rb.tick_log_count() == n and Rc.tick_log_count() == 0
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log: one call against twelve')
    assert ga.step_log_count() == gb.step_log_count() == gc.step_log_count() == 2 and gd.step_log_count() == 0
    la = ga.step_log()
    same_bytes(la, gb.step_log(), 'step log: one call against twelve')
    same_bytes(la, gc.step_log(), 'step log: one call against the chain')
    assert np.array_equal(la[:, :, 1], np.array([[5 * H] * B, [10 * H] * B]))
    assert not np.array_equal(sa['trajectory'], np.frombuffer(bytes(w.base.get_trajectory()), np.uint8))       # the updates moved the trajectories


def test_every_tick_record_is_the_read_back_of_its_tick(world):
    w = world
    log, chain = w.logged, w.chain
    assert log.shape == (kit.NTICKS, B, 64)
    assert_same(w._logged_end, w._chain_end, 'the logged call against the chain after %d ticks' % kit.NTICKS)
    for k, c in enumerate(chain):
        r = log[k]
        where = 'tick %d' % k
        assert np.all(r[:, F['tick']] == k) and np.all(r[:, F['time']] == k * H), where
        assert np.array_equal(r[:, F['targets_status']], c['status'][:, 0]) and np.array_equal(r[:, F['qp_status']], c['status'][:, 1] & 255), where
        assert np.array_equal(r[:, F['qp_iters']], c['status'][:, 1] >> 8), where
        same_bytes(r[:, F['base_pose']], c['q'][:, :7], where + ': base pose')
        same_bytes(r[:, F['base_twist']], c['v'][:, :6], where + ': base twist')
        same_bytes(r[:, F['torques']], c['control'][:, 24:], where + ': torques')
        same_bytes(r[:, F['contact_forces']], np.array([kit.unstack_forces(c['qp_sol'][b], c['contact'][b]).reshape(12) for b in range(B)]), where + ': forces')
        assert np.array_equal(r[:, F['contact']], c['contact']), where
        same_bytes(r[:, F['foot_heights']], c['ee'][:, :, 2], where + ': foot heights')
        same_bytes(r[:, F['base_accel']], c['qp_sol'][:, :6], where + ': base acceleration')
        assert np.all(r[:, 57:] == 0), where
        flags = r[:, F['flags']].astype(int)
        want_push = np.array([b == kit.PUSHED and k == kit.PUSH_TICK for b in range(B)])
        assert np.array_equal(flags & FLAG_PUSH != 0, want_push), where
        assert np.all((flags & FLAG_UPDATE != 0) == (k > 0 and k % TPU == 0)), where
        assert np.array_equal(flags & FLAG_COAST != 0, (c['status'][:, 1] & 255) > 1), where
    assert [k for k in range(kit.NTICKS) if int(log[k, 0, F['flags']]) & FLAG_UPDATE] == [5, 10, 15, 20, 25, 30]
    assert {tuple(r) for r in log[:, :, F['contact']].reshape(-1, 4).astype(int)} == {(0, 1, 1, 0), (1, 0, 0, 1)}       # the contact switch is inside


def test_the_plant_step_alone_against_the_restatement(world):
    """srbm_wb_plant_step_dev on seeded (q, v, a): solved and failed statuses, pushes on both ends of the tick, a rotation increment beyond 120
    degrees (the branch of the quaternion conversion with a non-positive trace).  q+ and v+ to 1e-9 (the bound test_gpu_mpc_period.py holds the
    single-rigid-body plant to), coast and push decisions exact"""
    w, m = world, world.model
    g, R = w.fresh(push=False)
    rng = np.random.default_rng(77)
    # QP status | iterations << 8: solved, solved to the reduced tolerances, max iterations, other; the targets status is not what decides
    status = np.array([[0, 0 | 9 << 8], [1, 1 | 12 << 8], [0, 2 | 200 << 8], [2, 8]], np.int32)
    for rnd, k in enumerate((0, 3, 41)):
        t_k = k * H
        q = w.q + rng.normal(size=(B, 19)) * 0.02
        q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
        v = rng.normal(size=(B, 18)) * 0.3
        if rnd == 2:
            v[1, 3:6] = [250.0, 20.0, -10.0]            # h |w| = 2.5 rad
        a = rng.normal(size=(B, 30)) * 5.0
        st = np.roll(status, rnd, axis=0)
        coast = (st[:, 1] & 255) > 1
        ptime = np.array([t_k + H, t_k, t_k + 0.5 * H, -1.0])      # fires at the end of the tick, not at its start, inside, never
        imp = rng.normal(size=(B, 6))
        want_push = np.array([True, False, True, False])
        assert [kit.push_applies(t_k, H, p) for p in ptime] == list(want_push)
        res = {}
        for pushed in (False, True):
            g.plant_set_push(ptime, imp) if pushed else g.plant_set_push()
            dq, dv, da, ds = Dev(q), Dev(v), Dev(a), Dev(st)
            R.plant_step_dev(k, H, dq.p.value, dv.p.value, da.p.value, ds.p.value)
            g.synchronize()
            res[pushed] = (dq.get(), dv.get())
        for b in range(B):
            where = 'round %d instance %d' % (rnd, b)
            # decisions, exact: a coasting instance without a push keeps its velocity to the bit; the push changes v+ of exactly the instances it hits
            assert np.array_equal(res[False][1][b], v[b]) == bool(coast[b]), where
            assert (not np.array_equal(res[True][1][b], res[False][1][b])) == bool(want_push[b]), where
            assert np.array_equal(res[True][1][b, 6:], res[False][1][b, 6:]), where
            for pushed in (False, True):
                qn, vn, p = kit.plant_step(q[b], v[b], a[b], H, k, m.mass, m.Ir_inv, coast[b], (ptime[b], imp[b]) if pushed else None)
                assert p == (pushed and want_push[b]), where
                eq, ev = np.abs(res[pushed][0][b] - qn).max(), np.abs(res[pushed][1][b] - vn).max()
                assert eq <= 1e-9 and ev <= 1e-9, (where, pushed, eq, ev)
    assert R.tick_log_count() == 0


def test_the_plant_is_the_whole_body_dynamics(world):
    """every logged tick whose QP solved: torques, forces and base acceleration of the log with the joint accelerations of the chain's qp_sol satisfy
    the 18 rows of M a + C v + g = S' tau + Js' F (wbc_numpy's RNEA and Jacobians) to 1e-6 max(1, |tau|_inf), the relative bound
    test_gpu_wbc.py holds the torques to.  No tick of an unpushed instance coasts (inputs chosen in test_controller_rollout_host.py)"""
    w, m = world, world.model
    log, chain = w.logged, w.chain
    worst, solved, coasted = 0.0, 0, 0
    for k, c in enumerate(chain):
        for b in range(B):
            r = log[k, b]
            if int(r[F['flags']]) & FLAG_COAST:
                coasted += b != kit.PUSHED
                continue
            assert r[F['qp_status']] <= 1
            solved += 1
            a = np.concatenate([r[F['base_accel']], c['qp_sol'][b, 6:18]])
            tau = r[F['torques']]
            res = kit.dynamics_residual(m, c['q'][b], c['v'][b], a, tau, r[F['contact_forces']].reshape(4, 3), r[F['contact']])
            rel = np.abs(res).max() / max(1.0, np.abs(tau).max())
            worst = max(worst, rel)
            assert rel <= 1e-6, (k, b, rel)
    # measured, not asserted (docs/history.md): the plant has no ground, so nothing holds these
    z = log[:, :, 8]
    ee = np.array([c['ee'] for c in chain])                      # [tick][B][4][3]
    con = log[:, :, F['contact']] > 0
    drift = 0.0
    for b in range(B):
        for e in range(4):
            ks = np.nonzero(con[:30, b, e])[0]                   # the first stance phase (up to the switch at tick 30)
            if len(ks):
                drift = max(drift, np.abs(ee[ks, b, e] - ee[ks[0], b, e]).max())
    print('dynamics residual: worst %.3g relative over %d solved ticks; coasted ticks of unpushed instances %d; base height %.4f .. %.4f; '
          'stance-foot drift over the first stance phase %.4f m' % (worst, solved, coasted, z.min(), z.max(), drift))
    assert coasted == 0 and solved >= 3 * kit.NTICKS


def test_against_the_restated_loop_resynchronised_before_every_tick():
    """2 instances x 6 ticks, an update every 3: before each tick the restatement's (q, v, q_des) are installed on the device and the trajectories
    are read back, so one tick's rounding never feeds the next.  qp_sol (base acceleration and forces from the log, all 18 accelerations through
    v+ - v) within test_gpu_wbc.py's 1e-6 relative, q+ to 1e-8 (the IK tests' bound on q), the state and ee handed to the solve at the update
    tick to 1e-9"""
    cfg = host.load_config('a1_configuration')
    model = kit.Model(cfg)
    rows = [0, kit.PUSHED]
    states, ees = instances(cfg, config_b_instance, rows)
    g = host.BatchMPC.cold_start(cfg, states, ees)
    q0 = np.tile(np.array(cfg['init_config'], float), (2, 1))
    qd, vd, _, st = g.get_targets_from_traj(0.0, q0)
    q, v = kit.first_measured(qd, vd)
    pt, imp = kit.pushes()
    pt, imp = pt[rows], imp[rows]
    R = ControllerRollout(g)
    g.plant_set_push(pt, imp)
    R.tick_log_enable(6); g.step_log_enable(2)
    loop = kit.RestatedLoop(model, g.get_trajectory(), q, v, q0, pt, imp)
    for k in range(6):
        loop.trajs = list(g.get_trajectory())
        R.reset(loop.q_des); R.set_state(loop.q, loop.v)
        v_before = loop.v.copy()
        out = loop.tick(k, H, 3)
        R.advance(k, 1, 3, H)
        qn, vn = R.state()
        rec = R.tick_log(k, 1)[0]
        for b, r in enumerate(out):
            where = 'tick %d instance %d' % (k, rows[b])
            assert r['targets_ok'] and not r['coast'] and rec[b, F['targets_status']] == 0 and rec[b, F['qp_status']] <= 1, where
            assert r['pushed'] == bool(int(rec[b, F['flags']]) & FLAG_PUSH) == (rows[b] == kit.PUSHED and k == kit.PUSH_TICK), where
            scale = max(1.0, np.abs(r['qp_sol']).max())
            ea = np.abs(rec[b, F['base_accel']] - r['qp_sol'][:6]).max() / scale
            ef = np.abs(rec[b, F['contact_forces']] - kit.unstack_forces(r['qp_sol'], r['contact']).reshape(12)).max() / scale
            edv = np.abs((vn[b] - v_before[b]) - (r['v_next'] - v_before[b])).max() / (H * scale)
            eq = np.abs(qn[b] - r['q_next']).max()
            print('%s: base accel %.3g forces %.3g (v+ - v) / h %.3g relative, q+ %.3g' % (where, ea, ef, edv, eq))
            assert ea <= 1e-6 and ef <= 1e-6 and edv <= 1e-6 and eq <= 1e-8, where
            assert np.array_equal(rec[b, F['contact']], r['contact']), where
        if k == 3:
            assert g.step_log_count() == 1
            s = g.step_log(0, 1)[0]
            for b, r in enumerate(out):
                assert s[b, 1] == 3 * H and np.abs(s[b, 17:30] - r['state']).max() <= 1e-9 and np.abs(s[b, 30:42] - r['ee'].reshape(12)).max() <= 1e-9, b
    assert g.step_log_count() == 1 and R.tick_log_count() == 6


def test_the_update_period(world):
    w = world
    before = np.frombuffer(bytes(w.base.get_trajectory()), np.uint8)
    g, R = w.fresh(step_log=8)
    R.advance(0, 12, 50, H)                  # the first update would follow tick 50
    g.synchronize()
    same_bytes(np.frombuffer(bytes(g.get_trajectory()), np.uint8), before, 'trajectories without an update')
    assert g.step_log_count() == 0
    g, R = w.fresh(step_log=8)
    R.advance(0, 6, 1, H)                    # an update after every tick but tick 0
    assert g.step_log_count() == 5
    log = g.step_log()
    same_bytes(log[:, :, 1], np.array([[k * H] * B for k in range(1, 6)]), 'init_time of the five solves')
    assert np.all(log[:, :, 0] == log[0, :, 0] + np.arange(5)[:, None])         # five solves in a row per instance


def test_summaries_of_a_rollout_fold_as_the_host_folds_them(world):
    w = world
    g, R = w.fresh(step_log=4)
    ref = rs.reference_from_config(w.cfg, B)
    crit = rs.criteria(z_min=0.2, tilt_max=0.5, r2_settle=1e-3, dz_settle=0.05, tilt_settle=0.05, h2_settle=1.0)
    rs.enable(g, crit, ref)
    R.advance(0, 12, TPU, H)
    rs.fold(g)
    got = rs.summaries(g)
    log = g.step_log()
    assert log.shape[0] == 2 and got[:, 0].tolist() == [2.0] * B
    mu = np.array([g.instance_model(b)[0].friction_coef for b in range(B)])
    same_bytes(got, rs.fold_host(g.L, log, crit, ref, mu), 'device fold against the host fold')


def test_refusals_leave_everything_untouched(world):
    w = world
    g, R = w.fresh(tick_log=4, step_log=1)
    R.advance(0, 2, TPU, H)
    g.synchronize()

    def state():
        return snapshot(w, g, R, 2), (R.tick_log_count(), g.step_log_count())
    s0, c0 = state()
    assert c0 == (2, 0)
    horizon = w.cfg['num_nodes'] * w.cfg['integrator_dt']
    cases = [((-1, 2, TPU, H), 'first_tick'), ((2, -1, TPU, H), 'ticks'), ((2, 2, 0, H), 'ticks_per_update'), ((2, 2, TPU, 0.0), 'tick_dt'),
             ((2, 2, TPU, -H), 'tick_dt'), ((2, 2, TPU, float('nan')), 'tick_dt'), ((2, 2, TPU, float('inf')), 'tick_dt'),
             ((2, 2, 100, H), 'MPC period'), ((2, 2, 1, horizon), 'MPC period'),
             ((2, 3, TPU, H), 'tick log has room for 2'),               # 2 of 4 slots left
             ((2, 2, 1, H), 'step log has room for 1')]                 # ticks 2 and 3 both update
    for args, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            R.advance(*args)
        s1, c1 = state()
        assert c1 == c0, args
        assert_same(s0, s1, 'after the refused call %s' % (args,))
    # what the batch lacks: plant state, q_des, whole-body model, leg kinematics
    c = w.base.clone()
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_state'):
        ControllerRollout(c).advance(0, 1, TPU, H)
    ControllerRollout(c).set_state(w.q, w.v)
    with pytest.raises(RuntimeError, match='srbm_control_tick_reset'):
        ControllerRollout(c).advance(0, 1, TPU, H)
    bare = host.BatchMPC({k: x for k, x in w.cfg.items() if k != 'body_model'}, B)
    Rb = ControllerRollout(bare)
    Rb.reset(w.q0); Rb.set_state(w.q, w.v)
    with pytest.raises(RuntimeError, match='whole-body model'):
        Rb.advance(0, 1, TPU, H)
    nolegs = host.BatchMPC({k: x for k, x in w.cfg.items() if k not in ('body_model', 'init_config', 'leg_origins')}, B)
    Rn = ControllerRollout(nolegs)
    Rn.reset(w.q0); Rn.set_state(w.q, w.v)
    with pytest.raises(RuntimeError, match='leg geometry'):
        Rn.advance(0, 1, TPU, H)
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_state'):
        ControllerRollout(w.base.clone()).state()
    # ... and the accepted call still runs from the untouched state: zero ticks are accepted and do nothing
    R.advance(2, 0, TPU, H)
    assert state()[1] == c0


def test_a_clone_carries_the_plant_and_has_logging_off(world):
    w = world
    g, R = w.fresh(tick_log=10, step_log=2)
    R.advance(0, 5, TPU, H)
    c = g.clone()
    Rc = ControllerRollout(c)
    assert Rc.tick_log_count() == 0 and c.step_log_count() == 0
    with pytest.raises(RuntimeError, match='no tick log'):
        Rc.tick_log(0, 0)
    R.advance(5, 5, TPU, H)
    Rc.advance(5, 5, TPU, H)                 # the push record and q_des went along; nothing is logged
    assert_same(snapshot(w, g, R, 10), snapshot(w, c, Rc, 10), 'clone after 5 ticks, 5 more')
    assert R.tick_log_count() == 10 and g.step_log_count() == 1 and Rc.tick_log_count() == 0          # (ticks 0 .. 9: the one update follows tick 5)
