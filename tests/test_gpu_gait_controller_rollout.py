"""The gait step in whole-controller rollouts (srbm_gait_controller_advance through ControllerRollout.advance(..., gait=, gait_opt_freq=)): the
update after tick k is run r = k / ticks_per_update of MPCController::MPCUpdate's branch -- line search, update + gradient + LP, plain update.

    1  gait_opt_freq 3 over one plain, one gradient and one line-search update: one call, one call per tick (a cut right before and right after
       every update, the line search's among them) and the host-driven chain of the tick entries and the public srbm_gait_* entries end bitwise
       equal; step-log fields 58..63 are the read-backs of srbm_gait_get_lp_result / srbm_gait_get_line_search_result.  Once on the torque-driven
       plant on a ground with contact feedback on (ticks 20 .. 27), once on the QP-acceleration plant (ticks 0 .. 7);
    2  with gait_opt_freq beyond the last update the entry is byte for byte srbm_controller_advance;
    3  the refusals, and the step-rule refusal of srbm_gait_compute_gradient after a rollout whose last solve ended by the step rule.

All batches run in the mode (0, 0), as tests/test_gpu_gait_closed_loop.py's: the host-driven chain cannot ask for the solve to the gap criterion."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import controller_rollout_kit as kit
from contact_feedback_kit import GroundWorld, flat_ground
from gpu_kit import same_bytes
from srbm_loader import gait_rollout, host
from srbm_loader.controller_rollout import ControllerRollout, PLANT_QP_ACCELERATION
from test_gpu_controller_rollout import World, Dev, snapshot, assert_same           # the kind-0 tests' batch and helpers

pytestmark = pytest.mark.gpu
B, H = kit.B, kit.TICK_DT
GF = gait_rollout.GAIT_LOG_FIELDS
PLAIN, GRADIENT, LINE_SEARCH = 0, 1, 2
TPU, FREQ, NT = 2, 3, 8


def kind_of(k):
    r = k // TPU
    return LINE_SEARCH if r % FREQ == 0 else GRADIENT if (r + 1) % FREQ == 0 else PLAIN


@pytest.fixture(scope='module')
def world():
    return World()


@pytest.fixture(scope='module')
def gw(world):
    return GroundWorld(world)


class Case:
    """'ground': kind 1 on a ground, feedback on, ticks 20 .. 27 (updates 10 plain, 11 gradient, 12 line search at t = 0.24, 13 plain);
    'kind0': the QP-acceleration plant, ticks 0 .. 7 (updates 1 plain, 2 gradient, 3 line search)"""

    def __init__(self, name, w, gw):
        self.name, self.w, self.gw = name, w, gw
        self.ground = name == 'ground'
        self.k0 = 20 if self.ground else 0
        self.q, self.v, _ = gw.start(self.k0)
        self.updates = [k for k in range(self.k0, self.k0 + NT) if k > 0 and k % TPU == 0]
        self.gr = flat_ground(gw, self.k0) if self.ground else None

    def fresh(self, **kw):
        if self.ground:
            g, R = self.gw.fresh(self.k0, self.gr, feedback=1, **kw)
        else:
            g, R = self.gw.fresh(self.k0, None, kind=PLANT_QP_ACCELERATION, **kw)
        return g, R, host.BatchGaitOptimizer(g)

    def snap(self, g, R, gait):
        s = ck.ground_snapshot(snapshot, self.w, g, R, self.k0 + NT)
        s['contact_times'], s['counts'] = gait.contact_times()
        return s


@pytest.mark.parametrize('name', ['ground', 'kind0'])
def test_one_call_one_call_per_tick_and_the_host_driven_chain_agree_bitwise(world, gw, name):
    w, c = world, Case(name, world, gw)
    n_upd = len(c.updates)
    assert {kind_of(k) for k in c.updates} == {PLAIN, GRADIENT, LINE_SEARCH}
    # (a) one call
    ga, Ra, gait_a = c.fresh(tick_log=NT, step_log=n_upd)
    Ra.advance(c.k0, NT, TPU, H, gait=gait_a, gait_opt_freq=FREQ)
    rec_a = ga.step_log()
    assert rec_a.shape == (n_upd, B, 64)
    # (b) one call per tick: after every update the record's fields 58..63 are the read-backs
    gb, Rb, gait_b = c.fresh(tick_log=NT, step_log=n_upd)
    roll_b = gait_rollout.GaitRollout(gb, gait_b)
    for k in range(c.k0, c.k0 + NT):
        Rb.advance(k, 1, TPU, H, gait=gait_b, gait_opt_freq=FREQ)
        if k not in c.updates:
            continue
        i = c.updates.index(k)
        assert gb.step_log_count() == i + 1
        rec = gb.step_log(i, 1)[0]
        assert np.all(rec[:, 1] == k * H), k
        expect = np.zeros((B, 6))
        if kind_of(k) == GRADIENT:
            lp_status, pred_red = gait_b.lp_result()
            valid = gait_b.gradient()[1]
            expect[:, 0], expect[:, 1], expect[:, 2], expect[:, 3] = 1, (valid == 1) & (lp_status == 0), lp_status, pred_red
            # the public line search of (c) cannot express "this instance was not ready": every instance must be
            assert np.all(rec[:, GF['ready']] == 1), (k, rec[:, 58:])
        elif kind_of(k) == LINE_SEARCH:
            imin, costs = roll_b.line_search_result()
            assert np.all((imin >= 0) & (imin < 10)), (k, imin)
            expect[:, 0], expect[:, 4], expect[:, 5] = 2, imin, costs[np.arange(B), imin]
        same_bytes(rec[:, 58:], expect, 'update after tick %d: fields 58..63' % k)
        assert not gb.status()[1].any(), k
    same_bytes(gb.step_log(), rec_a, 'step log: one call per tick against one call')
    same_bytes(Rb.tick_log(), Ra.tick_log(), 'tick log: one call per tick against one call')
    assert [int(x) for x in rec_a[:, 0, GF['kind']]] == [kind_of(k) for k in c.updates]

    # (c) the host-driven chain: the tick entries, then the public gait entries on what the tick wrote
    gc, Rc, gait_c = c.fresh()

    def update(k, state, t, ee):
        if kind_of(k) == LINE_SEARCH:
            imin, _ = gait_c.line_search(state, t, ee)
            same_bytes(imin.astype(float), rec_a[c.updates.index(k)][:, GF['imin']], 'imin of the public line search against the record')
        else:
            gc.get_real_time_update(state, t, ee)
            if kind_of(k) == GRADIENT:
                gait_c.compute_gradient()
                gait_c.optimize_contact_times(t)
    fb_c = ck.feedback_chain(Dev, gc, Rc, c.q, c.v, np.zeros((B, 4, 3)), c.k0, NT, TPU, feedback=c.ground, update=update, ground=c.ground)
    # (d) no logs
    gd, Rd, gait_d = c.fresh()
    Rd.advance(c.k0, NT, TPU, H, gait=gait_d, gait_opt_freq=FREQ)

    sa = c.snap(ga, Ra, gait_a)
    assert_same(sa, c.snap(gb, Rb, gait_b), 'one call per tick against one call')
    assert_same(sa, c.snap(gc, Rc, gait_c), 'the host-driven chain against one call')
    assert_same(sa, c.snap(gd, Rd, gait_d), 'without logs against with them')
    same_bytes(Ra.contact_feedback(), Rb.contact_feedback(), 'feedback record: one call per tick')
    same_bytes(Ra.contact_feedback(), fb_c, 'feedback record: the chain')
    # the gait step did something: the plain rollout ends on other trajectories
    ge, Re, _ = c.fresh()
    Re.advance(c.k0, NT, TPU, H)
    assert not np.array_equal(ck.traj_bytes(ge), sa['trajectory'])
    for gait in (gait_a, gait_b, gait_c, gait_d):
        gait.close()


@pytest.mark.parametrize('name', ['ground', 'kind0'])
def test_a_frequency_beyond_the_last_update_is_the_plain_entry(world, gw, name):
    w, c = world, Case(name, world, gw)
    ga, Ra, gait = c.fresh(tick_log=NT, step_log=len(c.updates))
    Ra.advance(c.k0, NT, TPU, H, gait=gait, gait_opt_freq=1000)
    gb, Rb, _ = c.fresh(tick_log=NT, step_log=len(c.updates))
    Rb.advance(c.k0, NT, TPU, H)
    assert_same(ck.ground_snapshot(snapshot, w, ga, Ra, c.k0 + NT), ck.ground_snapshot(snapshot, w, gb, Rb, c.k0 + NT), 'against srbm_controller_advance')
    same_bytes(Ra.tick_log(), Rb.tick_log(), 'tick log')
    same_bytes(ga.step_log(), gb.step_log(), 'step log')
    same_bytes(Ra.contact_feedback(), Rb.contact_feedback(), 'feedback record')
    assert not ga.step_log()[:, :, 58:].any()
    gait.close()


def test_refusals_and_the_step_rule(world, gw):
    w, c = world, Case('ground', world, gw)
    g, R, gait = c.fresh(tick_log=2, step_log=1)
    s0 = ck.ground_snapshot(snapshot, w, g, R, c.k0)
    cases = [((c.k0, 2, TPU, H, 0), 'gait_opt_freq'), ((c.k0, 2, TPU, H, -3), 'gait_opt_freq'), ((-1, 2, TPU, H, FREQ), 'first_tick'),
             ((c.k0, 2, 0, H, FREQ), 'ticks_per_update'), ((c.k0, 2, TPU, 0.0, FREQ), 'tick_dt'), ((c.k0, 2, 100, H, FREQ), 'MPC period'),
             ((c.k0, 3, TPU, H, FREQ), 'tick log has room for 2'), ((c.k0, 2, 1, H, FREQ), 'step log has room for 1')]
    for args, msg in cases:
        with pytest.raises(RuntimeError, match='srbm_gait_controller_advance.*' + msg):
            R.advance(*args[:4], gait=gait, gait_opt_freq=args[4])
        assert (R.tick_log_count(), g.step_log_count()) == (0, 0), args
        assert_same(s0, ck.ground_snapshot(snapshot, w, g, R, c.k0), 'after the refused call %s' % (args,))
    R.set_ground(None)                               # feedback is on: without a ground the gait entry refuses as the plain one does
    with pytest.raises(RuntimeError, match='srbm_controller_set_contact_feedback'):
        R.advance(c.k0, 2, TPU, H, gait=gait, gait_opt_freq=FREQ)
    other, _, other_gait = c.fresh()
    with pytest.raises(ValueError):
        R.advance(c.k0, 2, TPU, H, gait=other_gait, gait_opt_freq=FREQ)
    with pytest.raises(ValueError):
        R.advance(c.k0, 2, TPU, H, gait=gait)
    with pytest.raises(ValueError):
        R.advance(c.k0, 2, TPU, H, gait_opt_freq=FREQ)
    other_gait.close(); gait.close()
    # the step rule: the rollout takes the solve it differentiates to the gap criterion itself (srbm_gait_rti_advance does the same) and runs; a
    # gradient the CALLER asks for after a plain update that ended by the step rule is refused as before
    g, R, gait = c.fresh()
    g.set_solver_step_rule(host.FAST_TOL_STEP, 0.0)
    R.advance(c.k0, 3, TPU, H, gait=gait, gait_opt_freq=FREQ)          # ticks 20 .. 22: a plain update, then the gradient update
    g.synchronize()
    assert not g.status()[1].any()
    gait.compute_gradient()                          # the last solve ran to the gap criterion
    g2, R2, gait2 = c.fresh()
    g2.set_solver_step_rule(host.FAST_TOL_STEP, 0.0)
    R2.advance(c.k0, 1, TPU, H, gait=gait2, gait_opt_freq=FREQ)        # tick 20: a plain update under the step rule
    with pytest.raises(RuntimeError, match='step rule'):
        gait2.compute_gradient()
    gait.close(); gait2.close()
