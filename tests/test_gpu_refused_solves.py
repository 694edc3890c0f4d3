"""The gait step next to a solve that kernel 1 refused for capacity, and line searches of instances that are not ready (include/srbm_rti.h,
"Refused solves and the gait step"; csrc/srbm_gait_sens.hiph, srbm_gait_grad.hiph, srbm_gait_candidates.hiph).  Every assertion is an equality of
bits, flags or status words.

    1, 2  a batch whose middle instance was handed a schedule the build does not hold, through every public entry of the gait step: the
          neighbours are bit for bit those of a control batch, the refused instance has valid = 0, a zero gradient row, a zero sensitivity row and
          ten refused candidates, its trajectory untouched; once per capacity exit a schedule reaches (tests/refused_solves_kit.py), once on the
          LARGE build at N = 100
    3     the same through srbm_gait_rti_advance over a gradient run and the line search after it
    4     a rollout whose FIRST update is a line search, on a handle that never read contact times, is the plain entry bit for bit (open loop,
          closed loop, whole controller); the public srbm_gait_line_search refuses such a handle
    5     an instance that is not ready beside instances that search takes the plain update bit for bit (the re-applied contact-time formula
          would move interior knots of this state by a rounding: tests/test_refused_solves_host.py)
    6     srbm_export_qp and srbm_gait_get_param_partials refuse the refused instance and serve its neighbours

Beside every handle under test stands a bystander: a batch with a gait handle of its own, allocated after it, whose bytes must not move.
Batches are 3 instances of a1_configuration (N = 20) after tests/test_gpu_gait.py::run_pair's re-synchronised steps and one step of their own
from states that differ per instance."""
import numpy as np
import pytest

import contact_feedback_kit as ck
import refused_solves_kit as kit
from closed_loop_kit import SUB
from gpu_kit import same_bytes
from oracle_py import load_config
from srbm_loader import gait_rollout, host
from srbm_loader.workloads import EE_NOMINAL
from test_gpu_controller_rollout import World, snapshot
from test_gpu_gait import run_pair
from test_gpu_gait_controller_rollout import Case

pytestmark = pytest.mark.gpu
B, MID = 3, 1
NB = [b for b in range(B) if b != MID]
CAPACITY_BIT, OTHER = 16, 8
REFUSED = 'refused for capacity'


def record(g):
    """the instance records as the read-back entries show them, one row per instance"""
    st, err = g.status()
    z, s = g.dual_solution()
    return dict(status=st, err=err, sizes=g.sizes(), acc=g.status_accumulated(), states=g.trajectory_states(), x=g.qp_solution(),
                x_raw=g.raw_qp_minimiser(), z=z, s=s, stats=g.stats(), cost=g.qp_cost(),
                trajectory=np.frombuffer(bytes(g.get_trajectory()), np.uint8).reshape(g.batch, -1))      # knot times, kinds and values among it


def rows_same(a, b, rows, what):
    for k in a:
        same_bytes(a[k][rows], b[k][rows], '%s: %s of instances %s' % (what, k, rows))


def gait_arrays(gait):
    grad, valid = gait.gradient()
    lp_status, pred_red = gait.lp_result()
    xk, counts = gait.contact_times()
    return dict(gradient=grad, valid=valid, step=gait.step(), lp_status=lp_status, pred_red=pred_red, xk=xk, counts=counts)


class Bystander:
    """a batch and a gait handle allocated AFTER the handle under test, with something in every array; check(): nothing of it moved"""

    def __init__(self, src, time):
        self.g = src.clone()
        self.gait = host.BatchGaitOptimizer(self.g)
        self.gait.compute_gradient()
        self.gait.optimize_contact_times(time)
        self.before = self.snap()
        assert self.before['gradient'].any() and self.before['xk'].any()

    def snap(self):
        out = record(self.g)
        out.update(gait_arrays(self.gait))
        for b in range(self.g.batch):
            kn = self.g.knots(b)
            out['knot_times_%d' % b], out['knot_kinds_%d' % b] = kn['times'], kn['kinds']
        return out

    def check(self, what):
        after = self.snap()
        for k in self.before:
            same_bytes(after[k], self.before[k], '%s: the bystander batch: %s' % (what, k))


def own_times(g, mid_phase=None):
    """every instance's own contact times as srbm_update_contact_times takes them; with mid_phase the middle instance's are that far apart"""
    arr = np.zeros((g.batch, 4, 8))
    for b in range(g.batch):
        kn = g.knots(b)
        for e in range(4):
            nk = int(kn['nk'][e])
            ct = kn['times'][e, :nk][kn['kinds'][e, :nk] <= 1]
            arr[b, e, :len(ct)] = ct if (b != MID or mid_phase is None) else mid_phase * np.arange(len(ct))
    return arr


def next_inputs(g, t):
    """(state, t, ee) of a solve at t from the batch's own trajectories: node 1 and the planned foot locations"""
    return g.trajectory_states()[:, 1].copy(), t, g.eval_trajectory(t)[1]


class Base:
    """the batch every case clones, never modified: after run 3 (t = 0.15); `run` = 4 is the number of the next run"""

    def __init__(self, cfgname=kit.CFG, nsteps=kit.NSTEPS, large=False, **overrides):
        if large:
            self.cfg = load_config(cfgname, **overrides)
            s0 = np.array(self.cfg['srb_init'], float)
            self.g = host.BatchMPC.cold_start(self.cfg, [s0] * B, EE_NOMINAL, large=True, mode=(0.0, 0.0))
            self.run, state, ee = 0, np.tile(s0, (B, 1)), EE_NOMINAL
        else:
            self.cfg, self.g, o, _, _, _ = run_pair(cfgname, nsteps, batch=B)
            self.run, state, ee = nsteps, np.tile(o.states()[1], (B, 1)), kit.next_ee(o, nsteps * self.cfg['integrator_dt'])
        self.dt = self.cfg['integrator_dt']
        state[:, 0] += 0.004 * np.arange(B); state[:, 1] -= 0.003 * np.arange(B)           # no instance is a copy of its neighbour
        self.g.get_real_time_update(state, self.run * self.dt, ee)
        st, err = self.g.status()
        assert not err.any() and np.all(st == 0), (st, err)
        self.run += 1

    def time(self, run):
        return run * self.dt


@pytest.fixture(scope='module')
def base():
    return Base()


# ---- 1, 2: the gait step entry by entry ----
def entry_by_entry(base, phase, zero_step=False):
    """zero_step: the refused instance's step is set to zero before the line search.  Its LP minimised a zero gradient: the vertex it returns
    means nothing, and at PHASE_BOTH it moves candidates 5 .. 9 back inside the capacity (their solves are accepted and one of them wins: seen
    as statuses 8 8 8 8 8 0 0 0 0 0).  With a zero step its ten candidates are its own schedule."""
    mixed, control = base.g.clone(), base.g.clone()
    gm = host.BatchGaitOptimizer(mixed)
    by = Bystander(base.g, base.time(base.run))
    gc = host.BatchGaitOptimizer(control)
    state, t, ee = next_inputs(base.g, base.time(base.run))
    mixed.update_contact_times(own_times(mixed, phase)); control.update_contact_times(own_times(control))
    handed = record(mixed)
    mixed.get_real_time_update(state, t, ee); control.get_real_time_update(state, t, ee)
    rm, rc = record(mixed), record(control)
    assert rm['status'][MID] == OTHER and rm['err'][MID] & CAPACITY_BIT, (rm['status'], rm['err'])
    assert not rc['err'].any() and np.all(rc['status'] == 0) and not rm['err'][NB].any(), (rc['status'], rc['err'], rm['err'])
    rows_same(rm, rc, NB, 'after the update')
    for k in ('states', 'trajectory', 'x', 'z'):                   # a refused solve touches nothing of the trajectory or the last solution
        same_bytes(rm[k][MID], handed[k][MID], 'the refused instance after its update: %s' % k)

    gm.compute_sensitivity(); gc.compute_sensitivity()
    dm, dc = gm.sensitivity(), gc.sensitivity()
    same_bytes(dm[NB], dc[NB], 'sensitivity d of the neighbours')
    assert dc[MID].any() and not dm[MID].any()                     # (the header: a zero row for a refused instance)

    gm.compute_gradient(); gc.compute_gradient()
    gm.optimize_contact_times(t); gc.optimize_contact_times(t)
    am, ac = gait_arrays(gm), gait_arrays(gc)
    assert np.all(ac['valid'] == 1) and np.all(ac['lp_status'] == 0) and ac['gradient'][NB].any() and ac['step'][NB].any(), (ac['valid'], ac['lp_status'])
    for k in am:
        same_bytes(am[k][NB], ac[k][NB], 'after gradient and LP: %s of the neighbours' % k)
    assert am['valid'][MID] == 0 and not am['gradient'][MID].any()

    if zero_step:
        step = am['step'].copy(); step[MID] = 0.0
        gm.set_step(step)
        same_bytes(gm.step()[NB], ac['step'][NB], 'the step of the neighbours, written back')
    state2, t2, ee2 = next_inputs(control, base.time(base.run + 1))
    imin_m, costs_m = gm.line_search(state2, t2, ee2)
    imin_c, costs_c = gc.line_search(state2, t2, ee2)
    same_bytes(imin_m[NB], imin_c[NB], 'imin of the neighbours'); same_bytes(costs_m[NB], costs_c[NB], 'candidate costs of the neighbours')
    cst, cerr = gm.candidate_status()
    assert np.all(cerr[MID] & CAPACITY_BIT) and np.all(cst[MID] == OTHER) and not cerr[NB].any(), (cst, cerr)
    after = record(mixed)
    rows_same(after, record(control), NB, 'after the line search')
    assert after['status'][MID] == OTHER and after['err'][MID] & CAPACITY_BIT
    for k in ('states', 'trajectory'):
        same_bytes(after[k][MID], handed[k][MID], 'the refused instance after the line search: %s' % k)
    by.check('entry by entry')
    for gait in (gm, gc, by.gait):
        gait.close()


@pytest.mark.parametrize('phase,zero_step', [(kit.PHASE_VARIABLES, False), (kit.PHASE_BOTH, True)], ids=['spline_variables', 'variables_and_samples'])
def test_the_gait_step_entry_by_entry_beside_a_refused_instance(base, phase, zero_step):
    entry_by_entry(base, phase, zero_step)


def test_the_gait_step_beside_a_refused_instance_on_the_large_build():
    """N = 100, dt = 0.02 with the middle instance's contact times 0.2 s apart: n_u = 288 > 240
    (tests/test_gpu_dense_rows.py::test_large_build_capacity_overflow_fails_loudly)"""
    entry_by_entry(Base(large=True, num_nodes=100, integrator_dt=0.02), 0.2, zero_step=True)       # (as at PHASE_BOTH: statuses 8 8 8 8 8 0 0 0 0 0 without)


# ---- 3: through a rollout ----
def test_a_rollout_over_a_gradient_run_and_a_line_search_beside_a_refused_instance(base):
    F = base.run + 1                                               # run 4 is the gradient run, run 5 the line search
    mixed, control = base.g.clone(), base.g.clone()
    gm = host.BatchGaitOptimizer(mixed)
    by = Bystander(base.g, base.time(base.run))
    gc = host.BatchGaitOptimizer(control)
    mixed.update_contact_times(own_times(mixed, kit.PHASE_VARIABLES)); control.update_contact_times(own_times(control))
    gm.rti_advance(base.run, 1, F); gc.rti_advance(base.run, 1, F)
    mixed.synchronize(); control.synchronize()
    rm, rc = record(mixed), record(control)
    rows_same(rm, rc, NB, 'after the gradient run')
    assert rm['status'][MID] == OTHER and rm['err'][MID] & CAPACITY_BIT and not rc['err'].any()
    am, ac = gait_arrays(gm), gait_arrays(gc)
    assert np.all(ac['valid'] == 1) and np.all(ac['lp_status'] == 0), (ac['valid'], ac['lp_status'])
    for k in am:
        same_bytes(am[k][NB], ac[k][NB], 'after the gradient run: %s of the neighbours' % k)
    assert am['valid'][MID] == 0 and not am['gradient'][MID].any()
    gm.rti_advance(F, 1, F); gc.rti_advance(F, 1, F)
    mixed.synchronize(); control.synchronize()
    rm, rc = record(mixed), record(control)
    rows_same(rm, rc, NB, 'after the line-search run')
    imin_m, costs_m = gait_rollout.GaitRollout(mixed, gm).line_search_result()
    imin_c, costs_c = gait_rollout.GaitRollout(control, gc).line_search_result()
    assert np.all(imin_c >= 0), imin_c                             # every instance of the control batch was ready and searched
    same_bytes(imin_m[NB], imin_c[NB], 'imin of the neighbours'); same_bytes(costs_m[NB], costs_c[NB], 'candidate costs of the neighbours')
    assert imin_m[MID] == -1                                       # not ready: the plain update, refused again
    assert rm['status'][MID] == OTHER and rm['err'][MID] & CAPACITY_BIT
    by.check('the rollout')
    for gait in (gm, gc, by.gait):
        gait.close()


# ---- 4: the first update a line search, on a fresh handle ----
def no_capacity_bit(r):
    return not r['err'].any() and not (r['acc'][:, 0] & CAPACITY_BIT).any()


def test_a_first_update_that_is_a_line_search_is_the_plain_step_open_loop(base):
    F = base.run                                                   # run 4 of gait_opt_freq 4: a line-search run, and nothing is ready
    a, b = base.g.clone(), base.g.clone()
    gait = host.BatchGaitOptimizer(a)
    by = Bystander(base.g, base.time(base.run))
    gait.rti_advance(F, 1, F); a.synchronize()
    b.rti_advance(F, 1); b.synchronize()
    ra = record(a)
    rows_same(ra, record(b), list(range(B)), 'srbm_gait_rti_advance(F, 1, F) against srbm_rti_advance(F, 1)')
    assert no_capacity_bit(ra) and np.all(ra['status'] == 0), (ra['status'], ra['err'], ra['acc'])
    assert np.all(gait_rollout.GaitRollout(a, gait).line_search_result()[0] == -1)
    by.check('open loop')
    gait.close(); by.gait.close()


def test_a_first_update_that_is_a_line_search_is_the_plain_step_closed_loop(base):
    F = base.run
    a, b = base.g.clone(), base.g.clone()
    x0 = base.g.trajectory_states()[:, 0].copy()
    a.plant_set_state(x0); b.plant_set_state(x0)
    gait = host.BatchGaitOptimizer(a)
    by = Bystander(base.g, base.time(base.run))
    gait_rollout.GaitRollout(a, gait).advance(F, 1, F, SUB, True); a.synchronize()
    b.closed_loop_advance(F - 1, 1, SUB, True); b.synchronize()
    ra = record(a)
    rows_same(ra, record(b), list(range(B)), 'srbm_gait_closed_loop_advance(F, 1, F) against srbm_closed_loop_advance(F - 1, 1)')
    same_bytes(a.plant_state(), b.plant_state(), 'plant state')
    assert no_capacity_bit(ra) and np.all(ra['status'] == 0), (ra['status'], ra['err'], ra['acc'])
    assert np.all(gait_rollout.GaitRollout(a, gait).line_search_result()[0] == -1)
    by.check('closed loop')
    gait.close(); by.gait.close()


def test_a_first_update_that_is_a_line_search_is_the_plain_update_whole_controller():
    """ticks 20 .. 25 on the ground, an update every 2 ticks, gait_opt_freq 5: the update after tick 20 is run 10, a line-search run, the two
    after it are plain -- against srbm_controller_advance on the same batch"""
    w = World()
    c = Case('ground', w, ck.GroundWorld(w))
    tpu, freq, nt, H = 2, 5, 6, ck.H
    ga, Ra, gait = c.fresh()
    by = Bystander(ga, c.k0 * H)
    Ra.advance(c.k0, nt, tpu, H, gait=gait, gait_opt_freq=freq)
    gb, Rb, gait_b = c.fresh()
    Rb.advance(c.k0, nt, tpu, H)
    sa, sb = ck.ground_snapshot(snapshot, w, ga, Ra, c.k0 + nt), ck.ground_snapshot(snapshot, w, gb, Rb, c.k0 + nt)
    for k in sa:
        same_bytes(sa[k], sb[k], 'srbm_gait_controller_advance against srbm_controller_advance: %s' % k)
    ra = record(ga)
    rows_same(ra, record(gb), list(range(ga.batch)), 'srbm_gait_controller_advance against srbm_controller_advance')
    assert no_capacity_bit(ra), (ra['err'], ra['acc'])
    assert np.all(gait_rollout.GaitRollout(ga, gait).line_search_result()[0] == -1)
    by.check('whole controller')
    for g in (gait, gait_b, by.gait):
        g.close()


def test_the_public_line_search_refuses_a_handle_that_never_read_contact_times(base):
    g = base.g.clone()
    gait = host.BatchGaitOptimizer(g)
    before = record(g)
    state, t, ee = next_inputs(g, base.time(base.run))
    with pytest.raises(RuntimeError, match='srbm_gait_line_search.*srbm_gait_set_contact_times_from_trajectory'):
        gait.line_search(state, t, ee)
    rows_same(record(g), before, list(range(B)), 'after the refused line search')
    gait.set_contact_times_from_trajectory()
    imin, costs = gait.line_search(state, t, ee)                   # (step 0: ten copies of the plain schedule)
    assert np.all(imin >= 0) and not gait.candidate_status()[1].any()
    gait.close()


# ---- 5: a not-ready instance beside instances that search ----
DISPLACED = np.array([0.09, -0.06, -0.03])           # of the middle instance's plant: its feet leave their boxes, the QP of run 4 is primal infeasible (run 5's is solved)


def test_a_not_ready_instance_takes_the_plain_update_while_its_neighbours_search(base):
    """Closed loop, gait_opt_freq 5: run 4 is the gradient run, run 5 the line search.  The middle instance's plant stands DISPLACED from its
    trajectory: the QP of its gradient run is not Solved, the reference refuses the gradient (mpc.cpp:1048), the instance is not ready -- no
    error bit anywhere.  Its record after run 5 is that of a clone taken before run 5 and advanced by srbm_closed_loop_advance; its neighbours
    are those of a control batch whose middle instance stands on its trajectory and searches."""
    F = base.run + 1
    mixed, control = base.g.clone(), base.g.clone()
    x0 = base.g.trajectory_states()[:, 0].copy()
    xm = x0.copy(); xm[MID, :3] += DISPLACED
    mixed.plant_set_state(xm); control.plant_set_state(x0)
    gm = host.BatchGaitOptimizer(mixed)
    by = Bystander(base.g, base.time(base.run))
    gc = host.BatchGaitOptimizer(control)
    roll_m, roll_c = gait_rollout.GaitRollout(mixed, gm), gait_rollout.GaitRollout(control, gc)
    roll_m.advance(base.run, 1, F, SUB, True); roll_c.advance(base.run, 1, F, SUB, True)
    mixed.synchronize(); control.synchronize()
    rm, rc = record(mixed), record(control)
    am, ac = gait_arrays(gm), gait_arrays(gc)
    assert not rm['err'].any() and not rc['err'].any()
    assert np.all(ac['valid'] == 1) and np.all(ac['lp_status'] == 0), (ac['valid'], ac['lp_status'])
    assert rm['status'][MID] != 0 and list(am['valid']) == [1, 0, 1], (rm['status'], am['valid'])
    rows_same(rm, rc, NB, 'after the gradient run')
    twin = mixed.clone()
    roll_m.advance(F, 1, F, SUB, True); roll_c.advance(F, 1, F, SUB, True)
    twin.closed_loop_advance(F - 1, 1, SUB, True)
    mixed.synchronize(); control.synchronize(); twin.synchronize()
    rm, rc, rt = record(mixed), record(control), record(twin)
    rows_same(rm, rt, [MID], 'the not-ready instance against srbm_closed_loop_advance of a clone')
    same_bytes(mixed.plant_state()[MID], twin.plant_state()[MID], 'plant state of the not-ready instance')
    rows_same(rm, rc, NB, 'the neighbours after the line-search run')
    imin_m, costs_m = roll_m.line_search_result()
    imin_c, costs_c = roll_c.line_search_result()
    assert imin_m[MID] == -1 and np.all(imin_c >= 0), (imin_m, imin_c)
    same_bytes(imin_m[NB], imin_c[NB], 'imin of the neighbours'); same_bytes(costs_m[NB], costs_c[NB], 'candidate costs of the neighbours')
    assert not rm['err'].any() and not (rm['acc'][:, 0] & CAPACITY_BIT).any()
    by.check('a not-ready instance')
    for gait in (gm, gc, by.gait):
        gait.close()


# ---- 6: the debug exports ----
def test_the_exports_refuse_the_refused_instance_and_serve_its_neighbours(base):
    mixed, control = base.g.clone(), base.g.clone()
    state, t, ee = next_inputs(base.g, base.time(base.run))
    mixed.update_contact_times(own_times(mixed, kit.PHASE_VARIABLES)); control.update_contact_times(own_times(control))
    mixed.get_real_time_update(state, t, ee); control.get_real_time_update(state, t, ee)
    assert mixed.status()[0][MID] == OTHER and mixed.status()[1][MID] & CAPACITY_BIT
    with pytest.raises(RuntimeError, match='srbm_export_qp.*instance %d.*%s' % (MID, REFUSED)):
        mixed.export_qp(MID)
    with pytest.raises(RuntimeError, match='srbm_gait_get_param_partials.*instance %d.*%s' % (MID, REFUSED)):
        mixed.param_partials(MID, 0, 1)
    for b in NB:
        for name, xm, xc in zip('AbPq', mixed.export_qp(b), control.export_qp(b)):
            same_bytes(xm, xc, 'srbm_export_qp of neighbour %d: %s' % (b, name))
            assert xc.any()
        for name, xm, xc in zip(('dA', 'dG', 'db', 'dh'), mixed.param_partials(b, 0, 1), control.param_partials(b, 0, 1)):
            same_bytes(xm, xc, 'srbm_gait_get_param_partials of neighbour %d: %s' % (b, name))
    control.export_qp(MID); control.param_partials(MID, 0, 1)      # (the same instance on its own times: served)
