import importlib.util, os, sys, ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
from srbm_loader import host
host.LIB_PATH = os.path.join(ROOT, 'bilevel-gait-gen_amd', os.environ.get('SRBM_PROF_LIB', 'libsrbm_rti_prof.so'))
from srbm_loader import workloads as bench
cfg = host.load_config()
b = int(sys.argv[1]) if len(sys.argv) > 1 else 11
s0, ee = bench.config_b_instance(cfg, b)
g = host.BatchMPC.cold_start(cfg, s0, ee, mode=(float(os.environ['AB_STEP']), float(os.environ.get('AB_MU', 0))) if 'AB_STEP' in os.environ else None)
nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
for i in range(nsteps):
    g.rti_advance(i, 1)
g.synchronize()
print('counters', g.solver_counters()); print('status', g.status(), 'stats', g.stats()[0], 'sizes', g.sizes()[0])
name, traced, fields = C.c_char_p(), C.c_int(), []
for k in range(g.L.srbm_debug_trace_field(-1, None, None)): g.L.srbm_debug_trace_field(k, C.byref(name), C.byref(traced)); fields.append(name.value.decode())
rows = np.zeros((traced.value, len(fields)))         # one row per traced iteration
g.L.srbm_debug_get_trace(g.h, 0, rows.ctypes.data_as(C.POINTER(C.c_double)))
for it in range(min(int(g.stats()[0, 4]) + 1, len(rows))):
    print(it, ' '.join('%s %.4g' % nv for nv in zip(fields, rows[it])))
