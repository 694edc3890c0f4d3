"""Diagnostic: per-phase cycle shares of the IPM kernel (build with -DSRBM_PROFILE; never quote its run time); the coarse table: sums over the slot groups."""
import importlib.util, os, sys, ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location('srbm_host', os.path.join(ROOT, 'bilevel-gait-gen_amd', 'host.py'))
host = importlib.util.module_from_spec(spec); spec.loader.exec_module(host)
host.LIB_PATH = os.path.join(ROOT, 'bilevel-gait-gen_amd', 'libsrbm_rti_prof.so')
cfg = host.load_config(sys.argv[1] if len(sys.argv) > 1 else 'a1_configuration')
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
s0 = np.array(cfg['srb_init'], float)
ee = np.array([[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]], float)
mode = os.environ.get('PROF_MODE', 'lower_start')      # the mode bench.py's headline runs (round 5); 'step_rule' / 'ref' for the others
gb = host.BatchMPC.cold_start(cfg, [s0] * B, ee, mode={'lower_start': (0.0, host.FAST_START_MU), 'step_rule': (host.FAST_TOL_STEP, host.FAST_START_MU)}.get(mode),
                              initial_run=False)
print('solver settings', gb.solver_step_rule())

name, group = C.c_char_p(), C.c_char_p()
slots = []                                               # (name, group) of every cycle slot, as the library names them
for k in range(gb.L.srbm_debug_profile_slot(-1, None, None)):
    gb.L.srbm_debug_profile_slot(k, C.byref(name), C.byref(group)); slots.append((name.value.decode(), group.value.decode()))
groups = list(dict.fromkeys(g for _, g in slots))
def record():
    gb.synchronize(); out = np.zeros(len(slots)); gb.L.srbm_debug_get_profile(gb.h, 0, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out
gb.create_initial_run(s0, ee)
gb.rti_advance(0, 3)
before = record()
gb.rti_advance(3, 1)
last = record() - before                                 # the fourth RTI step alone
in_group = lambda g: [(n, v) for v, (n, gs) in zip(last, slots) if gs == g]
total = lambda g: sum(v for _, v in in_group(g))
ipm = [g for g in groups if g.startswith('ipm: ')]
tot = sum(total(g) for g in ipm)
print('iters', gb.stats()[0, 4], 'total stamp ticks %.0f' % tot)
for g in ipm:
    print('%-18s %10.0f  %5.1f%%' % (g[5:], total(g), 100 * total(g) / tot))
print('fine stamps (all of the last RTI step, as the table above; shares of its IPM solve):')
for g in groups:
    if g.startswith('step: '): print('%s, ticks: %.0f (%s)' % (g[6:], total(g), '; '.join('%s %.0f' % nv for nv in in_group(g))))
for g in ipm:
    for n, v in in_group(g): print('%-58s %12.0f %5.1f%%' % (n, v, 100 * v / tot))
