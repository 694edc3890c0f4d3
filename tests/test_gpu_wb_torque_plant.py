"""The torque-driven whole-body plant on the GPU (srbm_wb_plant_set_kind / _set_actuators / _set_bodies_each, srbm_wb_forward_dynamics,
srbm_wb_fd_step_dev; csrc/srbm_wb_fd.hiph through bilevel-gait-gen_amd/controller_rollout.py) against the numpy restatement of
tests/wb_torque_plant_kit.py: the solve alone, the identity with the controller, the plant step, the rollout three ways bit for bit and against the
restated loop, kind 0 untouched, the refusals and the clone.  The world is test_gpu_controller_rollout.py's: 4 Config-B instances after one cold
start, ticks of 10 ms (35 of them cross the first contact switch at 0.3 s), an MPC update every 5 ticks, instance 2 pushed in tick 3."""
import numpy as np
import pytest

import controller_rollout_kit as kit
import wb_torque_plant_kit as fd
from gpu_kit import same_bytes
from srbm_loader import host
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import (ControllerRollout, TICK_LOG_FIELDS, TORQUE_PLANT_LOG_FIELDS, FLAG_PUSH, FLAG_UPDATE, FLAG_COAST,
                                            FLAG_BREAKDOWN, PLANT_QP_ACCELERATION, PLANT_TORQUE_DRIVEN)
from srbm_loader.workloads import config_b_instance, instances
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same           # the kind-0 tests' batch and helpers

pytestmark = pytest.mark.gpu
B, H, TPU = kit.B, kit.TICK_DT, kit.TPU
F = dict(TICK_LOG_FIELDS, **TORQUE_PLANT_LOG_FIELDS)
HEAVY = 1               # the instance whose trunk is 20 % heavier than the controller's
WEAK = 3                # the instance whose torque limits are low enough to clamp


@pytest.fixture(scope='module')
def world():
    return World()


def rollout_actuators(cfg):
    """PD on, the configured torque bounds as limits, 8 Nm on every joint of instance WEAK"""
    lim = np.tile(np.asarray(cfg['torque_bounds'], float), (B, 1))
    lim[WEAK] = 8.0
    return np.full((B, 12), fd.KP), np.full((B, 12), fd.KD), lim


def heavy_bodies(cfg, batch=B, heavy=HEAVY):
    """per instance: the controller's bodies, the trunk of instance `heavy` 20 % heavier -> (body lists, restated models)"""
    lists = [fd.plant_cfg(cfg, 1.2 if b == heavy else 1.0)['body_model'] for b in range(batch)]
    return lists, [kit.Model(fd.plant_cfg(cfg, bodies=bl)) for bl in lists]


def torque_plant(w, R, kp, kd, lim, S, bodies=None):
    R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
    if bodies is not None:
        R.set_plant_bodies(*fd.bodies_arrays(bodies))


def run_fd_chain(g, R, q, v, first, ticks, tpu, h=H):
    """the loop driven from the host: srbm_control_tick_dev, srbm_wb_fd_step_dev, srbm_get_real_time_update_dev.  -> one dict per tick: the measured
    (q, v), every output of the tick, (a, F) of the plant's last sub-step"""
    T = ControlTick(g)
    n = g.batch
    d = dict(q=Dev(q), v=Dev(v), t=Dev(np.zeros(n)), control=Dev(np.zeros((n, 36))), qp_sol=Dev(np.zeros((n, 30))), status=Dev(np.zeros((n, 2), np.int32)),
             contact=Dev(np.zeros((n, 4), np.int32)), state=Dev(np.zeros((n, 13))), ee=Dev(np.zeros((n, 4, 3))), sol=Dev(np.zeros((n, 30))))
    out = []
    for k in range(first, first + ticks):
        g.synchronize()
        d['t'].put(np.full(n, k * h))
        rec = dict(q=d['q'].get(), v=d['v'].get())
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        R.fd_step_dev(k, h, d['q'].p.value, d['v'].p.value, d['control'].p.value, d['contact'].p.value, d['status'].p.value, d['sol'].p.value)
        if k > 0 and k % tpu == 0:
            g.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
        g.synchronize()
        rec.update({key: d[key].get() for key in ('control', 'qp_sol', 'status', 'contact', 'state', 'ee', 'sol')})
        out.append(rec)
    R.set_state(d['q'].get(), d['v'].get())          # the batch's own plant state is what the chain ended with (for snapshot)
    return out


def identity_bound(model, q, v, tau, contact, x_qp):
    """|x_plant - x_QP|_inf <= |K^-1|_inf rho + 1e-9 max(1, |x|_inf), rho the residual of the QP's (a, F) in the restated system K x = r"""
    K, r, _, _ = fd.kkt_system(model.robot, q, v, tau, contact)
    n = len(r)
    rho = np.abs(K @ x_qp[:n] - r).max()
    return np.abs(np.linalg.inv(K)).sum(axis=1).max() * rho + 1e-9 * max(1.0, np.abs(x_qp).max())


# ---- 1. the solve alone ----
def test_the_solve_alone_against_the_restatement():
    """srbm_wb_forward_dynamics on kit.solve_cases (every contact pattern, bases yawed and rolled past 90 degrees, |tau| up to the torque bounds), on
    the controller's bodies and on bodies of the plant's own: (a, F) within 1e-9 max(1, |x|_inf) of np.linalg.solve on the restated system, the
    dynamics residual within 1e-9 max(1, |tau|_inf); the device-pointer entry returns the same bytes; a NaN configuration gives status 1 and zeros"""
    cfg = host.load_config('a1_configuration')
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    worst_x = worst_r = 0.0
    controllers = kit.Model(cfg)
    for own in (False, True):
        models = [controllers] * B
        if own:
            lists = [fd.perturbed_bodies(cfg, b) for b in range(B)]
            R.set_plant_bodies(*fd.bodies_arrays(lists))
            models = [kit.Model(fd.plant_cfg(cfg, bodies=bl)) for bl in lists]
        for c, (q, v, tau, con) in enumerate(fd.solve_cases(cfg)):
            sol, st = R.forward_dynamics(q, v, tau, con)
            assert np.all(st == 0), (own, c, st)
            for b in range(B):
                where = 'own bodies %s call %d instance %d contact %s' % (own, c, b, con[b])
                want = fd.forward_dynamics(models[b].robot, q[b], v[b], tau[b], con[b])
                ex = np.abs(sol[b] - want).max() / max(1.0, np.abs(want).max())
                res = kit.dynamics_residual(models[b], q[b], v[b], sol[b, :18], tau[b], kit.unstack_forces(sol[b], con[b]), con[b])
                er = np.abs(res).max() / max(1.0, np.abs(tau[b]).max())
                worst_x, worst_r = max(worst_x, ex), max(worst_r, er)
                print('%s: (a, F) %.3g relative, dynamics residual %.3g relative' % (where, ex, er))
                assert ex <= 1e-9 and er <= 1e-9, where
                assert np.all(sol[b, 18 + 3 * int(con[b].sum()):] == 0), where
                if own:         # the bodies matter: the controller's give another answer
                    other = fd.forward_dynamics(controllers.robot, q[b], v[b], tau[b], con[b])
                    assert np.abs(sol[b] - other).max() > 1e-3, where
    print('worst over all cases: (a, F) %.3g relative, dynamics residual %.3g relative' % (worst_x, worst_r))
    q, v, tau, con = fd.solve_cases(cfg)[1]
    d = dict(q=Dev(q), v=Dev(v), tau=Dev(tau), con=Dev(con), sol=Dev(np.zeros((B, 30))), st=Dev(np.full(B, -1, np.int32)))
    R.forward_dynamics_dev(d['q'].p.value, d['v'].p.value, d['tau'].p.value, d['con'].p.value, d['sol'].p.value, d['st'].p.value)
    g.synchronize()
    sol, st = R.forward_dynamics(q, v, tau, con)
    same_bytes(d['sol'].get(), sol, 'the device-pointer entry against the host entry')
    assert np.array_equal(d['st'].get(), st)
    qn = q.copy(); qn[2, 9] = np.nan
    sol, st = R.forward_dynamics(qn, v, tau, con)
    assert st.tolist() == [0, 0, 1, 0] and np.all(sol[2] == 0) and np.all(np.isfinite(sol))


# ---- 2. identity with the controller ----
def test_the_plant_is_the_controllers_model_where_nothing_separates_them(world):
    """the forward dynamics under the QP's own torques on the controller's bodies returns the QP's (a, F) up to the QP's residual rho in the restated
    system: on four feet (the QP's stance rows are then the plant's and rho is the solver's tolerance: the instance with the heavier trunk exceeds
    the bound the matched ones keep), on the ticks of the kind-0 chain (bodies never set; in a trot the QP writes the right-hand side of the stance
    rows at the reference's foot-index rows, which rho then carries), and through log fields 61 and 62 of a kind-1 rollout with kp = kd = 0, no
    limits, S = 1"""
    w, m = world, world.model
    c0 = w.base.clone()
    R = ControllerRollout(c0)
    stand = np.ones((B, 4), np.int32)
    ctl, qsol, qst, _ = c0.qp_control(w.q, w.v, stand, w.q0, np.zeros(18), np.tile([0.0, 0.0, m.mass * 9.81 / 4], 4))
    assert np.all(qst <= 1)
    lists, _ = heavy_bodies(w.cfg)
    for heavy in (False, True):
        if heavy:
            R.set_plant_bodies(*fd.bodies_arrays(lists))
        sol, st = R.forward_dynamics(w.q, w.v, ctl[:, 24:], stand)
        for b in range(B):
            bound = identity_bound(m, w.q[b], w.v[b], ctl[b, 24:], stand[b], qsol[b])
            err = np.abs(sol[b] - qsol[b]).max()
            print('four feet, heavier trunk on instance %d %s, instance %d: |x_plant - x_QP| %.3g, bound %.3g' % (HEAVY, heavy, b, err, bound))
            assert st[b] == 0 and bound <= 1e-3 and (err > 100 * bound if heavy and b == HEAVY else err <= bound), (heavy, b, err, bound)
    R = ControllerRollout(w.base.clone())
    for k in (0, 7, 31):
        c = w.chain[k]
        sol, st = R.forward_dynamics(c['q'], c['v'], c['control'][:, 24:], c['contact'])
        for b in range(B):
            if (c['status'][b, 1] & 255) > 1:
                continue
            bound = identity_bound(m, c['q'][b], c['v'][b], c['control'][b, 24:], c['contact'][b], c['qp_sol'][b])
            err = np.abs(sol[b] - c['qp_sol'][b]).max()
            print('chain tick %d instance %d: |x_plant - x_QP| %.3g, bound %.3g' % (k, b, err, bound))
            assert st[b] == 0 and err <= bound, (k, b, err, bound)
    n = 12
    g, R = w.fresh(tick_log=n)
    torque_plant(w, R, np.zeros((B, 12)), np.zeros((B, 12)), np.full((B, 12), np.inf), 1, lists)
    ch = run_fd_chain(g, R, w.q, w.v, 0, n, TPU)
    g2, R2 = w.fresh(tick_log=n)
    torque_plant(w, R2, np.zeros((B, 12)), np.zeros((B, 12)), np.full((B, 12), np.inf), 1, lists)
    R2.advance(0, n, TPU, H)
    log = R2.tick_log()
    same_bytes(R2.state()[0], R.state()[0], 'the logged call against the chain')
    for k, c in enumerate(ch):
        for b in range(B):
            r = log[k, b]
            assert r[F['plant_kind']] == 1 and r[F['clamped_joints']] == 0 and r[F['torque_deviation']] == 0, (k, b)
            if (c['status'][b, 1] & 255) > 1:
                continue
            bound = identity_bound(m, c['q'][b], c['v'][b], c['control'][b, 24:], c['contact'][b], c['qp_sol'][b])
            if b == HEAVY:
                assert r[F['accel_mismatch']] > 0
                print('tick %d: the heavier instance: accel mismatch %.3g, identity bound %.3g' % (k, r[F['accel_mismatch']], bound))
            else:
                assert r[F['accel_mismatch']] <= bound and r[F['force_mismatch']] <= bound, (k, b, r[F['accel_mismatch']], r[F['force_mismatch']], bound)


# ---- 3. the step ----
def test_the_torque_plant_step_alone_against_the_restatement():
    """srbm_wb_fd_step_dev on kit.step_cases: S = 1 and 3, PD on, a joint driven into its limit, pushes on both ends of the tick and inside it, zero
    control actions (torque 0: the plant still falls).  q+, v+ and (a, F) of the last sub-step within 1e-9, push decisions exact"""
    cfg = host.load_config('a1_configuration')
    m = kit.Model(cfg)
    g = host.BatchMPC(cfg, B)
    R = ControllerRollout(g)
    kp, kd, lim = fd.step_actuators(cfg)
    clamped_somewhere = False
    for S in (1, 3):
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
        for rnd, c in enumerate(fd.step_cases(cfg, H)):
            off = (c['status'][:, 1] & 255) > 1
            res = {}
            for pushed in (False, True):
                g.plant_set_push(c['push_time'], c['impulse']) if pushed else g.plant_set_push()
                d = dict(q=Dev(c['q']), v=Dev(c['v']), ctl=Dev(c['control']), con=Dev(c['contact']), st=Dev(c['status']), sol=Dev(np.zeros((B, 30))))
                R.fd_step_dev(c['k'], H, d['q'].p.value, d['v'].p.value, d['ctl'].p.value, d['con'].p.value, d['st'].p.value, d['sol'].p.value)
                g.synchronize()
                res[pushed] = (d['q'].get(), d['v'].get(), d['sol'].get())
            for b in range(B):
                where = 'S %d round %d instance %d' % (S, rnd, b)
                assert (not np.array_equal(res[True][1][b], res[False][1][b])) == bool(c['want_push'][b]), where
                assert np.array_equal(res[True][1][b, 6:], res[False][1][b, 6:]), where
                same_bytes(res[True][2][b], res[False][2][b], where + ': (a, F) does not see the push')
                for pushed in (False, True):
                    push = (c['push_time'][b], c['impulse'][b]) if pushed else None
                    qn, vn, info = fd.fd_step(m.robot, c['q'][b], c['v'][b], c['control'][b], c['contact'][b], off[b], kp[b], kd[b], lim[b], H, S,
                                              c['k'], m.mass, m.Ir_inv, push)
                    assert info['pushed'] == (pushed and bool(c['want_push'][b])), where
                    eq, ev = np.abs(res[pushed][0][b] - qn).max(), np.abs(res[pushed][1][b] - vn).max()
                    es = np.abs(res[pushed][2][b] - info['sol']).max() / max(1.0, np.abs(info['sol']).max())
                    print('%s pushed %s: q+ %.3g v+ %.3g (a, F) %.3g relative' % (where, pushed, eq, ev, es))
                    assert eq <= 1e-9 and ev <= 1e-9 and es <= 1e-9, (where, pushed, eq, ev, es)
                    clamped_somewhere |= info['clamped'] > 0
                    if off[b]:        # the actuators are off and the robot is not held: it moves all the same
                        assert np.all(info['tau'] == 0) and np.abs(res[pushed][1][b] - c['v'][b]).max() > 1e-3, where
    assert clamped_somewhere
    assert R.tick_log_count() == 0


# ---- 4. the rollout ----
class Rollouts:
    """kind 1, S = 2, PD on, instance HEAVY with a trunk 20 % heavier, instance WEAK with low torque limits: the 35 ticks as a host-driven chain
    and as one logged call, computed once"""

    def __init__(self, w):
        self.w = w
        self.act = rollout_actuators(w.cfg)
        self.lists, self.models = heavy_bodies(w.cfg)
        self._chain = self._logged = None

    def fresh(self, **kw):
        g, R = self.w.fresh(**kw)
        torque_plant(self.w, R, *self.act, 2, self.lists)
        return g, R

    @property
    def chain(self):
        if self._chain is None:
            g, R = self.fresh(step_log=8)
            self._chain = run_fd_chain(g, R, self.w.q, self.w.v, 0, kit.NTICKS, TPU)
            self.chain_end = snapshot(self.w, g, R, kit.NTICKS)
            self.chain_steps = g.step_log()
        return self._chain

    @property
    def logged(self):
        if self._logged is None:
            g, R = self.fresh(tick_log=kit.NTICKS, step_log=8)
            R.advance(0, kit.NTICKS, TPU, H)
            self._logged = R.tick_log()
            self.logged_end = snapshot(self.w, g, R, kit.NTICKS)
            self.logged_steps = g.step_log()
        return self._logged


@pytest.fixture(scope='module')
def rollouts(world):
    return Rollouts(world)


def test_one_call_one_call_per_tick_and_the_host_driven_chain_bitwise(world, rollouts):
    w, n = world, 12
    ga, Ra = rollouts.fresh(tick_log=n, step_log=4)
    Ra.advance(0, n, TPU, H)
    gb, Rb = rollouts.fresh(tick_log=n, step_log=4)
    for k in range(n):
        Rb.advance(k, 1, TPU, H)
    gc, Rc = rollouts.fresh(step_log=4)
    run_fd_chain(gc, Rc, w.q, w.v, 0, n, TPU)
    sa = snapshot(w, ga, Ra, n)
    for name, g, R in (('one call per tick', gb, Rb), ('host-driven chain', gc, Rc)):
        assert_same(sa, snapshot(w, g, R, n), name)
    assert Ra.tick_log_count() == Rb.tick_log_count() == n and Rc.tick_log_count() == 0
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log: one call against one per tick')
    assert ga.step_log_count() == gb.step_log_count() == gc.step_log_count() == 2
    same_bytes(ga.step_log(), gb.step_log(), 'step log: one call against one per tick')
    same_bytes(ga.step_log(), gc.step_log(), 'step log: one call against the chain')
    # ... and the plant is not the other one: the same ticks with kind 0 end elsewhere
    g0, R0 = w.fresh()
    R0.advance(0, n, TPU, H)
    assert np.abs(R0.state()[0] - sa['q']).max() > 1e-6


def test_every_record_is_the_read_back_of_its_tick(world, rollouts):
    """the 35 ticks: fields 0..56 as the kind-0 log has them, 57..62 against the restated last sub-step on the chain's own control (the clamped count
    exact, the rest within 1e-9 relative), the heavier instance's mismatch"""
    w, ro = world, rollouts
    log, chain = ro.logged, ro.chain
    assert log.shape == (kit.NTICKS, B, 64)
    assert_same(ro.logged_end, ro.chain_end, 'the logged call against the chain after %d ticks' % kit.NTICKS)
    same_bytes(ro.logged_steps, ro.chain_steps, 'step log: the logged call against the chain')
    kp, kd, lim = ro.act
    clamped_ticks = 0
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
        flags = r[:, F['flags']].astype(int)
        assert np.array_equal(flags & FLAG_PUSH != 0, np.array([b == kit.PUSHED and k == kit.PUSH_TICK for b in range(B)])), where
        assert np.all((flags & FLAG_UPDATE != 0) == (k > 0 and k % TPU == 0)), where
        assert np.all(flags & (FLAG_COAST | FLAG_BREAKDOWN) == 0), where
        assert np.all(r[:, F['plant_kind']] == 1) and np.all(r[:, 63] == 0), where
        for b in range(B):
            off = (c['status'][b, 1] & 255) > 1
            # the last of the two sub-steps, restated from the chain's own outputs
            q1, v1, _ = fd.fd_step(ro.models[b].robot, c['q'][b], c['v'][b], c['control'][b], c['contact'][b], off, kp[b], kd[b], lim[b], H / 2, 1, 0,
                                   w.model.mass, w.model.Ir_inv)
            tau, clamped, dev = fd.torque_law(c['control'][b], q1, v1, kp[b], kd[b], lim[b], off)
            sol = fd.forward_dynamics(ro.models[b].robot, q1, v1, tau, c['contact'][b])
            nc = int(c['contact'][b].sum())
            want = (clamped, dev, sol[20:18 + 3 * nc:3].min() if nc else 0.0, np.abs(sol[:18] - c['qp_sol'][b, :18]).max(),
                    np.abs(sol[18:] - c['qp_sol'][b, 18:]).max())
            got = r[b, 58:63]
            assert got[0] == want[0], (where, b, got[0], want[0])
            for i in range(1, 5):
                assert abs(got[i] - want[i]) <= 1e-9 * max(1.0, abs(want[i])), (where, b, i, got[i], want[i])
            es = np.abs(c['sol'][b] - sol).max() / max(1.0, np.abs(sol).max())
            assert es <= 1e-9, (where, b, es)
            clamped_ticks += b == WEAK and clamped > 0
    assert clamped_ticks > 0
    assert [k for k in range(kit.NTICKS) if int(log[k, 0, F['flags']]) & FLAG_UPDATE] == [5, 10, 15, 20, 25, 30]
    assert len({tuple(r) for r in log[:, :, F['contact']].reshape(-1, 4).astype(int)}) >= 2                 # the contact switch is inside
    print('clamped ticks of instance %d: %d; accel mismatch: heavy %.3g, matched %.3g; smallest stance fz %.3g' % (
        WEAK, clamped_ticks, log[:, HEAVY, 61].max(), log[:, 0, 61].max(), log[:, :, 60].min()))


def test_against_the_restated_loop_resynchronised_before_every_tick():
    """2 instances x 6 ticks, an update every 3, as the host-driven chain (bit for bit the one-call rollout, above): before each tick the
    restatement's (q, v, q_des) are installed on the device and the trajectories are read back.  The tick's outputs (torques, qp_sol) within
    test_gpu_wbc.py's 1e-6 relative of the restated tick; the plant -- S = 2, PD on, the second instance's trunk 20 % heavier -- within 1e-9 of the
    restated step on the control action the device's tick returned (the torques of two QP solvers differ by more than the plant's bound)"""
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
    lists, pmodels = heavy_bodies(cfg, 2, 1)
    kp, kd, lim = np.full((2, 12), fd.KP), np.full((2, 12), fd.KD), np.tile(np.asarray(cfg['torque_bounds'], float), (2, 1))
    R = ControllerRollout(g)
    R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 2)
    R.set_plant_bodies(*fd.bodies_arrays(lists))
    g.plant_set_push(pt, imp)
    T = ControlTick(g)
    q_des = q0.copy()
    d = dict(q=Dev(q), v=Dev(v), t=Dev(np.zeros(2)), control=Dev(np.zeros((2, 36))), qp_sol=Dev(np.zeros((2, 30))), status=Dev(np.zeros((2, 2), np.int32)),
             contact=Dev(np.zeros((2, 4), np.int32)), state=Dev(np.zeros((2, 13))), ee=Dev(np.zeros((2, 4, 3))))
    for k in range(6):
        trajs = list(g.get_trajectory())
        R.reset(q_des)
        d['q'].put(q); d['v'].put(v); d['t'].put(np.full(2, k * H))
        T.tick_dev(d['q'].p.value, d['v'].p.value, d['t'].p.value, d['control'].p.value, d['qp_sol'].p.value, d['status'].p.value, None, None,
                   d['contact'].p.value, d['state'].p.value, d['ee'].p.value)
        R.fd_step_dev(k, H, d['q'].p.value, d['v'].p.value, d['control'].p.value, d['contact'].p.value, d['status'].p.value)
        if k > 0 and k % 3 == 0:
            g.get_real_time_update_dev(d['state'].p.value, d['t'].p.value, d['ee'].p.value)
        g.synchronize()
        ctl, sol, con, stt = d['control'].get(), d['qp_sol'].get(), d['contact'].get(), d['status'].get()
        qn, vn = d['q'].get(), d['v'].get()
        for b in range(2):
            where = 'tick %d instance %d' % (k, rows[b])
            r = kit.restated_tick(model, trajs[b], k * H, q[b], v[b], q_des[b])
            assert r['targets_ok'] and not r['coast'] and stt[b, 0] == 0 and (stt[b, 1] & 255) <= 1, where
            assert np.array_equal(con[b], r['contact']), where
            et = np.abs(ctl[b] - r['control']).max() / max(1.0, np.abs(r['control'][24:]).max())
            ex = np.abs(sol[b] - r['qp_sol']).max() / max(1.0, np.abs(r['qp_sol']).max())
            qr, vr, info = fd.fd_step(pmodels[b].robot, q[b], v[b], ctl[b], con[b], False, kp[b], kd[b], lim[b], H, 2, k, model.mass, model.Ir_inv,
                                      (pt[b], imp[b]))
            assert info['pushed'] == (rows[b] == kit.PUSHED and k == kit.PUSH_TICK), where
            eq, ev = np.abs(qn[b] - qr).max(), np.abs(vn[b] - vr).max()
            print('%s: control %.3g qp_sol %.3g relative, q+ %.3g v+ %.3g' % (where, et, ex, eq, ev))
            assert et <= 1e-6 and ex <= 1e-6 and eq <= 1e-9 and ev <= 1e-9, where
            q[b], v[b], q_des[b] = qr, vr, r['q_des']


# ---- 5. kind 0 untouched ----
def test_kind_0_with_the_new_settings_is_the_rollout_without_them(world):
    w, n = world, 12
    ga, Ra = w.fresh(tick_log=n, step_log=4)
    Ra.set_plant(PLANT_QP_ACCELERATION, *rollout_actuators(w.cfg), 3)
    Ra.set_plant_bodies(*fd.bodies_arrays([fd.perturbed_bodies(w.cfg, b) for b in range(B)]))
    Ra.advance(0, n, TPU, H)
    gb, Rb = w.fresh(tick_log=n, step_log=4)
    Rb.advance(0, n, TPU, H)
    assert_same(snapshot(w, ga, Ra, n), snapshot(w, gb, Rb, n), 'kind 0 with actuators and bodies set against a batch that never saw them')
    la = Ra.tick_log()
    same_bytes(la, Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    assert np.all(la[:, :, 57:] == 0)
    same_bytes(la, w.logged[:n], 'tick log against the kind-0 tests\' own')


# ---- 6. refusals and the clone ----
def test_refusals_leave_everything_untouched_and_a_clone_carries_the_settings(world, rollouts):
    w = world
    g, R = rollouts.fresh(tick_log=6, step_log=1)
    R.advance(0, 2, TPU, H)
    g.synchronize()
    twin = g.clone()                        # the settings as they are before the refused calls
    Rt = ControllerRollout(twin)
    assert Rt.tick_log_count() == 0 and twin.step_log_count() == 0
    with pytest.raises(RuntimeError, match='no tick log'):
        Rt.tick_log(0, 0)

    def state():
        return snapshot(w, g, R, 2), (R.tick_log_count(), g.step_log_count())
    s0, c0 = state()
    assert c0 == (2, 0)
    kp, kd, lim = rollouts.act
    mass, com, inertia = fd.bodies_arrays(rollouts.lists)

    def changed(a, idx, value):
        a = np.array(a, float); a[idx] = value
        return a
    cases = [(lambda: R.set_plant(2), 'kind 2'), (lambda: R.set_plant(-1), 'kind -1'),
             (lambda: R.set_plant(1, kp, kd, lim, 0), 'substeps'),
             (lambda: R.set_plant(1, changed(kp, (2, 5), -1.0), kd, lim, 2), 'instance 2, joint 5: kp'),
             (lambda: R.set_plant(1, changed(kp, (1, 0), np.nan), kd, lim, 2), 'instance 1, joint 0: kp'),
             (lambda: R.set_plant(1, kp, changed(kd, (3, 11), np.inf), lim, 2), 'instance 3, joint 11: kd'),
             (lambda: R.set_plant(1, kp, changed(kd, (0, 1), -0.5), lim, 2), 'instance 0, joint 1: kd'),
             (lambda: R.set_plant(1, kp, kd, changed(lim, (2, 2), np.nan), 2), 'instance 2, joint 2: the torque limit'),
             (lambda: R.set_plant(1, kp, kd, changed(lim, (0, 7), -1.0), 2), 'instance 0, joint 7: the torque limit'),
             (lambda: R.set_plant_bodies(changed(mass, (1, 4), 0.0), com, inertia), 'instance 1, body 4: the mass'),
             (lambda: R.set_plant_bodies(changed(mass, (3, 0), np.inf), com, inertia), 'instance 3, body 0: the mass'),
             (lambda: R.set_plant_bodies(mass, changed(com, (2, 12, 1), np.nan), inertia), 'instance 2, body 12: the centre of mass'),
             (lambda: R.set_plant_bodies(mass, com, changed(inertia, (0, 6, 1, 1), np.inf)), 'instance 0, body 6: the inertia')]
    for call, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            call()
        s1, c1 = state()
        assert c1 == c0, msg
        assert_same(s0, s1, 'after the refused call (%s)' % msg)
    # the settings are the ones from before: two more ticks end where the twin's end
    R.advance(2, 2, TPU, H)
    Rt.advance(2, 2, TPU, H)
    assert_same(snapshot(w, g, R, 4), snapshot(w, twin, Rt, 4), 'after the refused calls against the clone made before them')
    assert R.tick_log_count() == 4 and Rt.tick_log_count() == 0
    assert np.all(R.tick_log()[:, :, F['plant_kind']] == 1)
    # kind 1 without actuators: refused at the advance and at the step, the plant untouched
    c, Rc = w.fresh()
    Rc.set_plant(PLANT_TORQUE_DRIVEN)
    before = snapshot(w, c, Rc, 0)
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_actuators'):
        Rc.advance(0, 1, TPU, H)
    d = dict(q=Dev(w.q), v=Dev(w.v), ctl=Dev(np.zeros((B, 36))), con=Dev(np.ones((B, 4), np.int32)), st=Dev(np.zeros((B, 2), np.int32)))
    with pytest.raises(RuntimeError, match='srbm_wb_plant_set_actuators'):
        Rc.fd_step_dev(0, H, d['q'].p.value, d['v'].p.value, d['ctl'].p.value, d['con'].p.value, d['st'].p.value)
    same_bytes(d['q'].get(), w.q, 'the caller\'s q after the refused step')
    assert_same(before, snapshot(w, c, Rc, 0), 'after the refused advance')
    Rc.set_plant(PLANT_QP_ACCELERATION)
    Rc.advance(0, 1, TPU, H)                 # kind 0 needs none
    # forward dynamics without a whole-body model, without leg kinematics
    bare = host.BatchMPC({k: x for k, x in w.cfg.items() if k != 'body_model'}, B)
    with pytest.raises(RuntimeError, match='whole-body model'):
        ControllerRollout(bare).forward_dynamics(w.q, w.v, np.zeros((B, 12)), np.ones((B, 4), int))
    nolegs = host.BatchMPC({k: x for k, x in w.cfg.items() if k not in ('body_model', 'init_config', 'leg_origins')}, B)
    with pytest.raises(RuntimeError, match='leg geometry'):
        ControllerRollout(nolegs).forward_dynamics(w.q, w.v, np.zeros((B, 12)), np.ones((B, 4), int))
