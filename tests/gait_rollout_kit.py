"""The controller loop with the gait step closed over the plant, on the CPU restatement: what tests/test_gpu_gait_closed_loop.py holds
srbm_gait_closed_loop_advance to (a plain module: nothing pytest collects).  One run is plant_integrate -> push -> ee_value at t -> rti /
rti + gait_gradient + gait_optimize / gait_line_search, branched on the run number as controllers/mpc_controller.cpp:320-346."""
import numpy as np

from oracle_py import OracleMPC

PLAIN, GRADIENT, LINE_SEARCH = 0, 1, 2


class RestatementLoop:
    """one instance after its cold start; run() performs run number self.next_run.  Before a run, self.o holds the trajectory and self.x the plant
    state the run starts from (what a re-synchronised device is given)."""

    def __init__(self, cfg, state, ee, freq, substeps, advance_time, push_time, impulse):
        self.cfg, self.freq, self.substeps, self.advance_time = cfg, freq, substeps, advance_time
        self.push_time, self.impulse = push_time, np.asarray(impulse, float)
        self.o = OracleMPC(cfg); self.o.set_warmstart(state); self.o.initial_run(state, ee)
        self.x = np.array(state, float)
        self.ready = False
        self.next_run = 1

    def run(self):
        """-> dict(run, t, plant (after integration and push), ee, kind, ready (after the run), step (LP step of a gradient run that is ready, else
        None), imin, costs (of a line-search run that searched, else None))"""
        o, r, F, dt = self.o, self.next_run, self.freq, self.cfg['integrator_dt']
        t0 = (r - 1) * dt
        t = t0 + dt                                             # (the device forms the time of run r the same way)
        x = o.plant_integrate(self.x, t0, dt / self.substeps, self.substeps, self.advance_time)
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
