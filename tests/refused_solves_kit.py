"""What tests/test_refused_solves_host.py and tests/test_gpu_refused_solves.py share: the contact schedules that make kernel 1 refuse a solve
for capacity, with the sizes the CPU oracle gives them (its vectors grow: it solves what the device refuses), and a numpy restatement of
srbm_apply_contact_times (csrc/srbm_gait_candidates.hiph; EndEffectorSplines::SetContactTimes, end_effector_splines.cpp:860-892).
A plain module: no fixtures, nothing pytest collects.

The state of every case: a1_configuration (N = 20, dt = 0.05) after NSTEPS re-synchronised open-loop RTI steps from srb_init
(tests/test_gpu_gait.py::run_pair) and one more step at t = 0.15, every foot with five contact times 0.3 s apart.  A schedule is `phase`: the
contact times of a foot set to phase * (0, 1, 2, ...), as tests/test_gpu_parity.py::test_capacity_overflow_fails_loudly sets them, and solved at the
next node time, t = 0.2.  (The 50 ms phases of that test overflow at t = 0; at t = 0.2 four of their five contact times are in the past and
n_u is 148: they fit.)

Which of kernel 1's three capacity exits (csrc/srbm_k1_assemble.hiph) such a schedule reaches, at the standard build's 160 spline variables,
120 force samples and 32 knots per foot (test_refused_solves_host.py holds every line to the oracle):
    spline variables alone      phase 0.06: n_u 176, 120 samples (not more than 120), 16 knots per foot
    force samples               never alone: a sampled stance phase brings 10 samples and 12 force variables, so 130 samples come with 156
                                force variables and the position variables beside them; phase 0.07 trips both (n_u 204, 140 samples)
    knots per foot              not reached: five contact times per foot are 11 knots, and the horizon extension adds phases of at least
                                0.2 s up to a window of 1 s -- the grid's largest table has 19 knots, the exit needs 30"""
import numpy as np

from oracle_py import OracleMPC, load_config
from srbm_loader.workloads import EE_NOMINAL

CFG, NSTEPS = 'a1_configuration', 3
CAPACITY = dict(nu=160, samples=120, knots=32)                 # the standard build (srbm_get_capacity)
PHASE_VARIABLES, PHASE_BOTH = 0.06, 0.07
GRID = (0.02, 0.03, 0.05, 0.06, 0.07, 0.1, 0.15, 0.2)           # uniform phases searched for an exit reached alone


def reach_oracle(cfgname=CFG, nsteps=NSTEPS + 1):
    """the oracle after nsteps open-loop RTI steps -> (cfg, oracle, the time of its last solve)"""
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    o = OracleMPC(cfg)
    o.set_warmstart(s0)
    o.initial_run(s0, EE_NOMINAL)
    t = 0.0
    for i in range(nsteps):
        t = i * cfg['integrator_dt']
        o.rti(o.states()[1], t, next_ee(o, t))
    return cfg, o, t


def next_ee(o, t):
    return np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])


def uniform_times(counts, phase):
    return [phase * np.arange(int(k)) for k in counts]


def oracle_sizes(o, t_next, times):
    """(n_u, force samples, knots of the longest table) of the RTI step at t_next on a copy of the oracle given the contact times `times`"""
    c = o.clone()
    c.set_contact_times(times)
    c.rti(c.states()[1], t_next, next_ee(c, t_next))
    sz = c.sizes()
    return sz['n'] - 12 * (c.N + 1), sz['n_force_box'] // 2, max(c.knots(e)['K'] for e in range(4))


def exits(nu, samples, knots, cap=CAPACITY):
    """which capacity exits of kernel 1 those sizes reach (the knot exit: no room for three more knots while the horizon is extended)"""
    return {k for k, hit in (('nu', nu > cap['nu']), ('samples', samples > cap['samples']), ('knots', knots > cap['knots'])) if hit}


def knot_kinds(kn):
    """the device's knot kinds of an oracle table (OracleMPC.knots): LO 0, TD 1, stance-interior 2, mid-swing 3"""
    return np.array([int(tt) if tt < 2 else (2 if int(ft) == 1 else 3) for tt, ft in zip(kn['ttypes'], kn['ftype'][0])])


def reapply_contact_times(times, kinds):
    """srbm_apply_contact_times with the table's OWN contact times: every operation in the device's order, one rounding each"""
    ct = [0.0 if (t < 0 and abs(t) < 1e-3) else float(t) for t, k in zip(times, kinds) if k <= 1]
    out = np.array(times, dtype=np.float64)
    c = 0
    for i, k in enumerate(kinds):
        if k <= 1:
            out[i] = ct[c]; c += 1
        elif k == 3:
            d = ct[c] - ct[c - 1]
            h = d / 2
            out[i] = out[i - 1] + h
        else:
            contact_time = 0.2 + ct[c - 1]
            if c < len(ct):
                contact_time = ct[c] - ct[c - 1]
            h = contact_time / 3
            out[i] = out[i - 1] + h
    return out
