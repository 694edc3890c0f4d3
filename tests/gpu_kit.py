"""What the GPU tests and the developer scripts share beyond the package's own helpers (workloads.instances, workloads.EE_NOMINAL,
BatchMPC.cold_start): tolerances, comparisons and small drivers.  A plain module: no fixtures, nothing pytest collects.

    REL_TOL, relerr             every parity module (parity, resync, gait, large, ownpath, closed_loop, mpc_period, instance_params, dense_rows;
                                gpu_protocols, closed_loop_kit), test_lp_reference_host
    EE_TEST                     test_gpu_parity, test_oracle_mpc
    status_ok_or_bad            test_gpu_parity (there as status_class), test_gpu_mpc_period
    status_four_classes         gpu_protocols.resync_protocol (there as cls)
    advance, snapshot,
    assert_bitwise              gpu_protocols.run_case, test_gpu_step_log
    same_bytes                  test_gpu_step_log, test_gpu_gait_lp, test_gpu_gait_closed_loop, test_gpu_mpc_period, closed_loop_kit (assert_same);
                                through assert_rows_bitwise: test_gpu_instance_params
    wbc_inputs                  test_gpu_wbc, scripts/dev_prof_wbc.py

The two long drivers (run_case, make_batch / resync_protocol) are in tests/gpu_protocols.py; what the closed-loop tests share (the CPU restatement
of the loop, its inputs, the comparisons of two batches) is in tests/closed_loop_kit.py."""
import ctypes as C

import numpy as np

from oracle_py import load_config

REL_TOL = 1e-4          # stated tolerance of the north star
EE_TEST = np.array([[0.1526, 0.12523, 0.011089], [0.1526, -0.12523, 0.011089],
                    [-0.208321844, 0.1363286, 0.01444], [-0.208321844, -0.1363286, 0.01444]])  # test/mpc_test.cpp:97-101


def relerr(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def status_ok_or_bad(st):
    """Solved / SolvedInacc / MaxIter steer MPCSingleRigidBody::Solve identically (msrb.cpp:136-144); which of the three
    an interior-point code reports at a 1e-15 gap tolerance is solver-internal (Clarabel is unpinned)."""
    return 'ok' if int(st) in (0, 1, 2) else 'bad'


def status_four_classes(v):
    v = int(v)
    return 'solved' if v <= 1 else ('maxiter' if v == 2 else ('infeasible' if v in (3, 5) else 'other'))


def advance(g, closed, first, steps):
    if closed:
        g.closed_loop_advance(first, steps)
    else:
        g.rti_advance(first, steps)


def snapshot(g, closed):
    st, err = g.status()
    z, s = g.dual_solution()
    it = np.zeros(g.batch)
    g._chk(g.L.srbm_debug_get_instance_iters(g.h, it.ctypes.data_as(C.POINTER(C.c_double))))
    c = g.solver_counters()
    out = dict(sizes=g.sizes(), status=st, err=err, acc=g.status_accumulated(), flags=g.solve_flags(),
               solver_counters=np.array([c['solves'], c['step_rule'], c['low_tried'], c['low_failed']]), work_counters=np.array(g.work_counters()),
               instance_iters=it, stats=g.stats(), x=g.qp_solution(), x_raw=g.raw_qp_minimiser(), z=z, s=s, states=g.trajectory_states(),
               trajectory=bytes(g.get_trajectory()))
    if closed:
        out['plant'] = g.plant_state()
    return out


def assert_bitwise(a, b, where):
    for k in a:
        if isinstance(a[k], bytes):
            assert a[k] == b[k], '%s: %s differs' % (where, k)
        elif a[k].tobytes() != b[k].tobytes():
            diff = (a[k].view(np.uint8) != b[k].view(np.uint8)).reshape(len(a[k]), -1).any(axis=1) if a[k].ndim > 1 else a[k] != b[k]
            raise AssertionError('%s: %s differs at %s %s' % (where, k, 'instances' if a[k].ndim > 1 else 'entries', np.nonzero(diff)[0][:8].tolist()))


def same_bytes(a, b, what):
    """two arrays of one shape hold the same bytes; the message names the first differing elements by index (for records of the step log:
    step, instance, field)"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a != b) if a.itemsize != b.itemsize else np.argwhere(
            (np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).reshape(a.shape + (a.itemsize,)).any(axis=-1))
        raise AssertionError('%s: differs at %s' % (what, bad[:8].tolist()))


def assert_rows_bitwise(a, ia, b, ib, where):
    """row ia of every array of dict a against row ib of dict b"""
    for k in a:
        same_bytes(a[k][ia], b[k][ib], '%s: %s (instance %d against row %d)' % (where, k, ia, ib))


def wbc_inputs(B, seed=3):
    """seeded inputs of the whole-body QP around the nominal configuration: (cfg, q, v, q_des, v_des, rng)"""
    cfg = load_config()
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    q = np.tile(q0, (B, 1))
    q[:, :3] += rng.normal(size=(B, 3)) * 0.03
    quat = q[:, 3:7] + np.concatenate([rng.normal(size=(B, 3)) * 0.05, np.zeros((B, 1))], axis=1)
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    q[:, 7:] += rng.normal(size=(B, 12)) * 0.1
    v = rng.normal(size=(B, 18)) * 0.1
    q_des = np.tile(q0, (B, 1)); q_des[:, 7:] += rng.normal(size=(B, 12)) * 0.02
    v_des = rng.normal(size=(B, 18)) * 0.05
    return cfg, q, v, q_des, v_des, rng
