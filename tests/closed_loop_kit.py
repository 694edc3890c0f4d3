"""What the closed-loop tests share (test_gpu_closed_loop, test_gpu_gait_closed_loop, test_gpu_mpc_period, test_mpc_period_host; chip_cu_count also
test_gpu_step_log and test_gpu_instance_params).  A plain module like gpu_kit.py: no fixtures, nothing pytest collects.

    RestatementLoop, PLAIN, GRADIENT,       the controller loop closed over the plant on the CPU restatement: what the device is held to
    LINE_SEARCH, NO_GAIT
    IMPULSES, PUSH, PUSH_TIMES, push_draw,  the inputs, each stated once (tests/test_mpc_period_host.py holds the cases to their conditions on the
    SUB, GAIT_FREQ, GAIT_RUNS,              restatement alone)
    PLAIN_CASES, plain_case, GAIT_CASES
    MODE, rollout, end_state, assert_same,  the device side: the solver mode of the gait-loop and period batches, a batch's gait rollout, what two
    chip_cu_count, step_queues_on_and_off   batches are compared in, the chip's CU count, the in-process switch of the step queues
    resync_gait_loop                        the gait loop against the restatement, re-synchronised before every run

One run of the restatement is plant_integrate -> push -> ee_value at t -> rti / rti + gait_gradient + gait_optimize / gait_line_search, branched on the
run number as controllers/mpc_controller.cpp:320-346.  It takes any time: orc_mpc_rti and orc_mpc_plant_integrate are handed t and p / substeps exactly
as the device forms them (include/srbm_rti.h, srbm_plant_set_period):

    time = (r - 1) * p;  x <- CalcIntegral(x, trajectory, time, substeps steps of p / substeps);  push if time < push_time <= time + p;
    solve at time + p with the foot locations of the trajectory at time + p
"""
import numpy as np

from gpu_kit import REL_TOL, relerr, same_bytes
from oracle_py import OracleMPC, load_config
from srbm_loader import gait_rollout, host, mpc_period, workloads

PLAIN, GRADIENT, LINE_SEARCH = 0, 1, 2
NO_GAIT = 10 ** 9            # a gait_opt_freq no run number reaches: every run is a plain one
MODE = (0.0, 0.0)


# ---- the restatement ----
class RestatementLoop:
    """one instance after its cold start; run() performs run number self.next_run at the MPC period (None: the node step; gait_opt_freq counts runs
    either way).  Before a run, self.o holds the trajectory and self.x the plant state the run starts from (what a re-synchronised device is given)."""

    def __init__(self, cfg, state, ee, freq, substeps, advance_time, push_time, impulse, period=None):
        self.cfg, self.freq, self.substeps, self.advance_time = cfg, freq, substeps, advance_time
        self.push_time, self.impulse = push_time, np.asarray(impulse, float)
        self.period = float(cfg['integrator_dt'] if period is None else period)
        self.o = OracleMPC(cfg); self.o.set_warmstart(state); self.o.initial_run(state, ee)
        self.x = np.array(state, float)
        self.ready = False
        self.next_run = 1

    def run(self):
        """-> dict(run, t, plant (after integration and push), ee, kind, ready (after the run), step (LP step of a gradient run that is ready, else
        None), imin, costs (of a line-search run that searched, else None))"""
        o, r, F, p = self.o, self.next_run, self.freq, self.period
        t0 = (r - 1) * p
        t = t0 + p                                              # (the device forms the time of run r the same way)
        x = o.plant_integrate(self.x, t0, p / self.substeps, self.substeps, self.advance_time)
        if t0 < self.push_time <= t:
            x[3:6] += self.impulse[:3]; x[10:13] += self.impulse[3:]
        eev = np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])
        out = dict(run=r, t=t, plant=x.copy(), ee=eev, step=None, imin=None, costs=None)
        if r % F == 0 and self.ready:
            out['imin'], out['costs'] = o.gait_line_search(x, t, eev)
            out['kind'] = LINE_SEARCH
            self.ready = False
        elif r % F != 0 and (r + 1) % F == 0:
            o.rti(x, t, eev)
            out['kind'] = GRADIENT
            try:
                self.ready = o.gait_gradient() is not None
                if self.ready:
                    out['step'], _ = o.gait_optimize(t)
            except RuntimeError:                                # the sensitivity system not factorised / "Bad gait optimization solve"
                self.ready = False
                out['step'] = None
        else:
            o.rti(x, t, eev)
            out['kind'] = PLAIN
            self.ready = False
        out['ready'] = self.ready
        self.x = x
        self.next_run = r + 1
        return out


# ---- the inputs ----
# three impulse rows for config_b instances 0..2 (instance 2 is never pushed: its row never arrives), then the push of the gait loops
IMPULSES = np.array([[2.5, -1.0, 0.3, 0.05, -0.1, 0.2], [-1.5, 2.0, 0.0, 0.0, 0.1, -0.1], [9, 9, 9, 9, 9, 9], [1.5, -1.0, 0.2, 0.03, -0.05, 0.1]], float)
PUSH = IMPULSES[3]
PUSH_TIMES = np.array([0.12, 0.07, 1e9, 0.03])
SUB = 4
# plain loop: name -> (configuration, instance generator of workloads, periods, push times, runs, advance_time values)
PLAIN_CASES = {
    'config_b': ('a1_configuration', 'config_b_instance', np.array([0.05, 0.025, 0.013, 0.0171]), PUSH_TIMES, 24, (0, 1)),
    'config_d': ('a1_config_distr_rejection', 'config_d_instance', np.array([0.02, 0.007, 0.031]), np.array([0.03, 0.02, 1e9]), 12, (1,)),
}
# gait loop (srb_init, EE_NOMINAL, PUSH, freq 5, 11 runs): (configuration, push time, period)
GAIT_CASES = [('a1_configuration', 0.03, 0.013), ('a1_gait_opt_config', 0.05, 0.03)]
GAIT_FREQ, GAIT_RUNS = 5, 11


def plain_case(name):
    """-> (cfg, states[B][13], ees[B][4][3], periods[B], push_times[B], impulses[B][6], runs, advance_time values)"""
    cfgname, gen, periods, push_times, runs, adv = PLAIN_CASES[name]
    cfg = load_config(cfgname)
    B = len(periods)
    states, ees = workloads.instances(cfg, getattr(workloads, gen), B)
    return cfg, states, np.asarray(ees).reshape(B, 4, 3), periods, push_times, IMPULSES[:B], runs, adv


def push_draw():
    """the pushes of the eight-instance batches, drawn per instance -> (push_times[8], impulses[8][6], the generator after the draw)"""
    rng = np.random.default_rng(5)
    return rng.uniform(0.0, 0.3, 8), rng.normal(0, 1.0, (8, 6)) * np.array([2.5, 2.5, 0.5, 0.2, 0.2, 0.2]), rng


# ---- the device side ----
def rollout(g, log=0):
    """the gait optimiser and the rollout of a batch whose plant is set; log: room for that many runs"""
    if log:
        g.step_log_enable(log)
    gait = host.BatchGaitOptimizer(g)
    return gait, gait_rollout.GaitRollout(g, gait)


def end_state(g, gait=None, records=False):
    st, err = g.status()
    out = dict(plant=g.plant_state(), states=g.trajectory_states(), x=g.qp_solution(), status=st, err=err, sizes=g.sizes(),
               trajectory=np.frombuffer(bytes(g.get_trajectory()), np.uint8))           # (the knot tables among it)
    if gait is not None:
        out['contact_times'], out['counts'] = gait.contact_times()
    if records:
        out['records'] = g.step_log()
    return out


def assert_same(a, b, what, keys=None):
    for k in keys or a:
        same_bytes(a[k], b[k], '%s: %s' % (what, k))


def chip_cu_count():
    probe = host.BatchMPC(load_config(), 1)
    n_cu = probe.debug_launch_info()['n_cu']
    probe.close()
    return n_cu


def step_queues_on_and_off(monkeypatch):
    """yields no_queue = False, then True, with SRBM_NO_STEP_QUEUE set to match (the switch is read when a batch is created)"""
    for no_queue in (False, True):
        if no_queue:
            monkeypatch.setenv('SRBM_NO_STEP_QUEUE', '1')
        else:
            monkeypatch.delenv('SRBM_NO_STEP_QUEUE', raising=False)
        yield no_queue


# ---- the re-synchronised gait loop ----
def resync_gait_loop(cfgname, push_time, period=None):
    """Two identical instances, 11 runs, a push, at the MPC period (None: no setting, the node step).  Before every run the device is given the
    restatement's trajectory and plant state, after a gradient run its LP step.  Per run: no error bits, the two instances on the same bytes,
    plant <= 1e-9 (identical records in: the project's own figure for one plant step is 1e-12), node states < REL_TOL, knot tables equal, init_time
    of the record == (r - 1) * p + p, kind; ready flag and LP status of a gradient run; the argmin of a line search whose two cheapest candidates are
    more than 1e-4 apart -- which both line searches must be."""
    cfg = load_config(cfgname)
    p = cfg['integrator_dt'] if period is None else period
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, workloads.EE_NOMINAL, mode=MODE)
    g.plant_set_state(s0); g.plant_set_push(push_time, PUSH)
    if period is not None:
        mpc_period.plant_set_period(g, period)
    gait, roll = rollout(g, log=GAIT_RUNS)
    loop = RestatementLoop(cfg, s0, workloads.EE_NOMINAL, GAIT_FREQ, SUB, 1, push_time, PUSH, period)
    n_ls = n_argmin = 0
    for r in range(1, GAIT_RUNS + 1):
        g.set_warm_start_trajectory([loop.o.trajectory_record(host)] * 2)
        g.plant_set_state(loop.x)
        out = loop.run()
        roll.advance(r, 1, GAIT_FREQ, SUB, True); g.synchronize()
        if out['step'] is not None:
            nv = int(gait.contact_times()[1][0].sum())
            gait.set_step(out['step'][:nv])
        st, err = g.status()
        assert not err.any(), (r, err)
        plant, tr = g.plant_state(), g.trajectory_states()
        e_plant, e_tr = relerr(plant[0], out['plant']), relerr(tr[0], loop.o.states())
        print('%s p = %g run %2d kind %d: plant %.1e states %.1e' % (cfgname, p, r, out['kind'], e_plant, e_tr))
        assert np.array_equal(plant[0], plant[1]) and np.array_equal(tr[0], tr[1]), r
        assert e_plant <= 1e-9, (r, e_plant)
        assert e_tr < REL_TOL, (r, e_tr)
        kg = g.knots(0)
        same_bytes(np.frombuffer(bytes(g.get_trajectory(0, 1)), np.uint8), np.frombuffer(bytes(g.get_trajectory(1, 1)), np.uint8), 'run %d: the two instances' % r)
        for e in range(4):
            ko = loop.o.knots(e)
            assert kg['nk'][e] == ko['K'] and np.array_equal(kg['times'][e, :ko['K']], ko['times']), (r, e)
        rec = g.step_log(r - 1, 1)[0]
        same_bytes(rec[0], rec[1], 'run %d: the records of the two instances' % r)
        same_bytes(rec[:, 1], np.full(2, (r - 1) * p + p), 'run %d: init_time of the record' % r)
        fields = gait_rollout.gait_fields_from_log(rec[0])
        assert fields['kind'] == out['kind'], (r, fields, out['kind'])
        if out['kind'] == GRADIENT:
            assert fields['ready'] == int(out['ready']) == 1 and fields['lp_status'] == 0, (r, fields)
        if out['kind'] == LINE_SEARCH:
            n_ls += 1
            imin, costs = roll.line_search_result()
            assert imin[0] == imin[1] == fields['imin']
            srt = np.sort(out['costs'])
            print('   line search: device imin %d, restatement %d; its two cheapest candidates %.3e apart (relative)' %
                  (imin[0], out['imin'], (srt[1] - srt[0]) / max(1.0, abs(srt[0]))))
            if srt[1] - srt[0] > 1e-4 * max(1.0, abs(srt[0])):
                n_argmin += 1
                assert imin[0] == out['imin'], (r, imin[0], out['imin'], costs[0], out['costs'])
    assert n_ls == 2 and n_argmin == 2, (n_ls, n_argmin)
    gait.close(); g.close()
