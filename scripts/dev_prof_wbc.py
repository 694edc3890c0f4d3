"""Cycles per phase of the whole-body QP solve (diagnostic build: make -C bilevel-gait-gen_amd/csrc ../libsrbm_rti_prof.so; run with
SRBM_RTI_LIB=bilevel-gait-gen_amd/libsrbm_rti_prof.so).  The stamps come back in the last row of A of the QP dump (free with < 4 feet in contact)."""
import os, sys, ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from srbm_loader import host
from gpu_kit import wbc_inputs

B = 256
cfg, q, v, q_des, v_des, rng = wbc_inputs(B, seed=9)
contact = np.array([[[1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 0]][b % 3] for b in range(B)], np.int32)
fdes = np.zeros((B, 12))
for b in range(B):
    nc = contact[b].sum(); fdes[b, :3 * nc] = np.tile([0, 0, cfg['mass'] * 9.81 / nc], nc)
g = host.BatchMPC(cfg, B)
ctl, sol, st, iters, qp = g.qp_control(q, v, contact, q_des, v_des, fdes, dump=True)
# the 'wbc: ' slots as the library names them, in slot order: the order of the stamps in the dump
name, group, slots = C.c_char_p(), C.c_char_p(), []
for k in range(g.L.srbm_debug_profile_slot(-1, None, None)):
    g.L.srbm_debug_profile_slot(k, C.byref(name), C.byref(group))
    if group.value.startswith(b'wbc: '): slots.append((name.value.decode(), group.value.decode()))
pr = qp['A'][:, -1, :len(slots)]
tot = sum(pr[:, k] for k, (_, grp) in enumerate(slots) if grp == 'wbc: solve')
print('iterations min %d median %d max %d; statuses %s' % (iters.min(), np.median(iters), iters.max(), np.unique(st, return_counts=True)))
print('whole solve (cycles of s_memtime): mean %.0f max %.0f' % (tot.mean(), tot.max()))
for k, (nme, grp) in enumerate(slots):
    if grp == 'wbc: solve': print('%-22s mean %9.0f  share %5.1f %%   per iteration %8.0f' % (nme, pr[:, k].mean(), 100 * pr[:, k].sum() / tot.sum(), (pr[:, k] / np.maximum(1, iters)).mean()))
    else: print('%s (%s: dynamics by 20 recursive Newton-Euler passes, rows, split): mean %.0f max %.0f' % (nme, grp[5:], pr[:, k].mean(), pr[:, k].max()))
