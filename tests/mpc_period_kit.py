"""The closed loop at an MPC period other than the node step, on the CPU restatement: what tests/test_gpu_mpc_period.py holds the device to, and the
inputs both period test files share (a plain module: nothing pytest collects).  The restatement takes any time: orc_mpc_rti and
orc_mpc_plant_integrate are handed t and p / substeps exactly as the device forms them (include/srbm_rti.h, srbm_plant_set_period):

    time = (r - 1) * p;  x <- CalcIntegral(x, trajectory, time, substeps steps of p / substeps);  push if time < push_time <= time + p;
    solve at time + p with the foot locations of the trajectory at time + p
"""
import numpy as np

from gait_rollout_kit import GRADIENT, LINE_SEARCH, PLAIN, RestatementLoop

NO_GAIT = 10 ** 9            # a gait_opt_freq no run number reaches: every run is a plain one


class PeriodLoop(RestatementLoop):
    """RestatementLoop with the MPC period p in place of the node step; gait_opt_freq keeps counting runs"""

    def __init__(self, cfg, state, ee, freq, substeps, advance_time, push_time, impulse, period):
        super().__init__(cfg, state, ee, freq, substeps, advance_time, push_time, impulse)
        self.period = float(period)

    def run(self):
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


# ---- the inputs of the period tests (chosen on the restatement alone: tests/test_mpc_period_host.py holds them to their conditions) ----
# the three impulse rows of tests/test_gpu_closed_loop.py, then the push of tests/test_gpu_gait_closed_loop.py
IMPULSES = np.array([[2.5, -1.0, 0.3, 0.05, -0.1, 0.2], [-1.5, 2.0, 0.0, 0.0, 0.1, -0.1], [9, 9, 9, 9, 9, 9], [1.5, -1.0, 0.2, 0.03, -0.05, 0.1]], float)
PUSH = IMPULSES[3]
SUB = 4
# plain loop: name -> (configuration, instance generator of workloads, periods, push times, runs, advance_time values)
PLAIN_CASES = {
    'config_b': ('a1_configuration', 'config_b_instance', np.array([0.05, 0.025, 0.013, 0.0171]), np.array([0.12, 0.07, 1e9, 0.03]), 24, (0, 1)),
    'config_d': ('a1_config_distr_rejection', 'config_d_instance', np.array([0.02, 0.007, 0.031]), np.array([0.03, 0.02, 1e9]), 12, (1,)),
}
# gait loop (srb_init, EE_NOMINAL, PUSH, freq 5, 11 runs): (configuration, push time, period)
GAIT_CASES = [('a1_configuration', 0.03, 0.013), ('a1_gait_opt_config', 0.05, 0.03)]
GAIT_FREQ, GAIT_RUNS = 5, 11


def plain_case(name):
    """-> (cfg, states[B][13], ees[B][4][3], periods[B], push_times[B], impulses[B][6], runs, advance_time values)"""
    from oracle_py import load_config
    from srbm_loader import workloads
    cfgname, gen, periods, push_times, runs, adv = PLAIN_CASES[name]
    cfg = load_config(cfgname)
    B = len(periods)
    states, ees = workloads.instances(cfg, getattr(workloads, gen), B)
    return cfg, states, np.asarray(ees).reshape(B, 4, 3), periods, push_times, IMPULSES[:B], runs, adv
