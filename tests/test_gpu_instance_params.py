"""Per-instance model constants and costs within one batch (srbm_batch_create_each, the _each cost setters, BatchMPC.from_configs).

Every instance of a heterogeneous batch must be exactly the reference object its own config describes.  Without a tolerance: each instance of a
batch of different objects is held BIT FOR BIT to a batch of one made from its config alone (BatchMPC(cfg_b, 1)) on every launch path -- the
fused K-step launch in both solver modes, the step queues of a batch larger than the chip, the closed-loop plant, the gait line search (whose
candidate c of instance b solves with instance b's record), the whole-body targets and the LARGE build.  With the oracle: 32 instances on
identical inputs against OracleMPC(cfg_b).  The heterogeneous set: the Config-B instances (workloads.config_b_instance) with mass +-15 %, Ir
scaled by 0.8 .. 1.2, friction 0.5 / 0.6, force bound 150 / 200, force cost 0 / 1e-3, the Q diagonal of a1_configuration or
a1_config_distr_rejection, a target with x, y in [0, 1] and height 0.28 .. 0.34, and on one instance a full symmetric positive-definite Q."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from closed_loop_kit import chip_cu_count
from cost_variants_kit import cost_set, install, spd
from gpu_kit import REL_TOL, assert_rows_bitwise, relerr
from oracle_py import OracleMPC, load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, heterogeneous_configs, instances

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_Q_INST = 3          # the instance of a heterogeneous set whose tracking and final costs are a full SPD matrix


def het_configs(B, seed=4242, num_nodes=None):
    return heterogeneous_configs(load_config('a1_configuration'), [load_config(n)['Q_srbd_diag'] for n in ('a1_configuration', 'a1_config_distr_rejection')],
                                 B, seed, num_nodes)


def full_q(cfg):
    """a full symmetric positive-definite Q around the config's diagonal (fixed seed)"""
    return spd(cfg, 99)


def full_q_costs(cfg):
    """(des, Q, Phi, Phi_w) of the full-Q instance, as setup() installs them"""
    Q, des = full_q(cfg), host.manifold_to_tangent(cfg['srb_target'])
    return des, Q, Q, -1 * Q @ des


def inputs(cfgs):
    return instances(cfgs, config_b_instance, len(cfgs))


def setup(g, mode, states, ees, full=()):
    """full: (index within g, cfg) pairs whose costs become the full-Q costs"""
    for k, cfg in full:
        install(g, k, [full_q_costs(cfg)])
    g.set_state_trajectory_warm_start(states)
    g.set_solver_tolerances(*host.REFERENCE_SOLVER_SETTINGS)
    g.set_solver_step_rule(*mode)
    g.create_initial_run(states, ees)


def make_het(cfgs, mode, large=None, full=True):
    states, ees = inputs(cfgs)
    g = host.BatchMPC.from_configs(cfgs, large=large)
    setup(g, mode, states, ees, [(FULL_Q_INST, cfgs[FULL_Q_INST])] if full and len(cfgs) > FULL_Q_INST else [])
    return g, states, ees


def make_one(cfgs, b, mode, large=None, full=True):
    states, ees = inputs(cfgs)
    g = host.BatchMPC(cfgs[b], 1, large=large)
    setup(g, mode, states[b:b + 1], ees[b:b + 1], [(0, cfgs[b])] if full and b == FULL_Q_INST else [])
    return g


def snap(g):
    """every per-instance output, one row per instance (the set tests/test_gpu_launch_equivalence.py compares, batch totals excepted)"""
    st, err = g.status()
    z, s = g.dual_solution()
    it = np.zeros(g.batch)
    g._chk(g.L.srbm_debug_get_instance_iters(g.h, it.ctypes.data_as(C.POINTER(C.c_double))))
    out = dict(sizes=g.sizes(), status=st, err=err, acc=g.status_accumulated(), flags=g.solve_flags(), instance_iters=it, stats=g.stats(),
               x=g.qp_solution(), x_raw=g.raw_qp_minimiser(), z=z, s=s, states=g.trajectory_states())
    tr = g.get_trajectory()
    out['trajectory'] = np.array([np.frombuffer(bytes(t), np.uint8) for t in tr])
    return out


# ---- 1. batch of one equivalence ----
@pytest.mark.parametrize('mode', [(0.0, 0.0), (0.0, 0.1)])
def test_heterogeneous_batch_is_bitwise_its_batches_of_one(mode):
    cfgs = het_configs(8)
    g, _, _ = make_het(cfgs, mode)
    g.rti_advance(0, 10); g.synchronize()
    a = snap(g)
    assert np.all(a['err'] == 0)
    # the set is heterogeneous where it matters: different constructor data give different plans
    assert len({a['x'][b].tobytes() for b in range(8)}) == 8
    for b in range(8):
        o = make_one(cfgs, b, mode)
        o.rti_advance(0, 10); o.synchronize()
        assert_rows_bitwise(a, b, snap(o), 0, 'mode %s' % (mode,))
        o.close()
    g.close()


# ---- 2. the step queues ----
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_gpu_instance_params as T
B, steps, path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
g, _, _ = T.make_het(T.het_configs(B), (0.0, 0.1))
g.rti_advance(0, steps); g.synchronize()
info = g.debug_launch_info()
np.savez(path, queued=np.array(info['queued']), **T.snap(g))
'''


def run_child(B, steps, no_queue, path):
    env = dict(os.environ)
    env.pop('SRBM_NO_STEP_QUEUE', None)
    if no_queue:
        env['SRBM_NO_STEP_QUEUE'] = '1'
    p = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests')), str(B), str(steps), path], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = np.load(path)
    return bool(d['queued']), {k: d[k] for k in d.files if k != 'queued'}


def test_queued_heterogeneous_batch_is_bitwise_the_per_instance_launch():
    n_cu = chip_cu_count()
    B, steps = n_cu + 8, 3
    with tempfile.TemporaryDirectory() as tmp:
        queued, a = run_child(B, steps, False, os.path.join(tmp, 'q.npz'))
        plain, b = run_child(B, steps, True, os.path.join(tmp, 'p.npz'))
    assert queued and not plain
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    cfgs = het_configs(B)
    for i in (0, FULL_Q_INST, n_cu // 2 + 1, B - 1):
        o = make_one(cfgs, i, (0.0, 0.1))
        o.rti_advance(0, steps); o.synchronize()
        assert_rows_bitwise(a, i, snap(o), 0, 'queued launch')
        o.close()


# ---- 3. the oracle on identical inputs ----
def test_heterogeneous_batch_matches_its_oracles_on_identical_inputs():
    B, steps = 32, 12
    cfgs = het_configs(B)
    states, ees = inputs(cfgs)
    g = host.BatchMPC.cold_start(cfgs, states, ees, mode=(0.0, 0.0), initial_run=False)
    install(g, FULL_Q_INST, [full_q_costs(cfgs[FULL_Q_INST])])               # the full-Q instance faces its oracle like every other
    g.create_initial_run(states, ees)
    oracles = [OracleMPC(c) for c in cfgs]
    oracles[FULL_Q_INST].set_costs(*full_q_costs(cfgs[FULL_Q_INST]))
    for b, o in enumerate(oracles):
        o.set_warmstart(states[b])
    pool = ThreadPoolExecutor(16)
    list(pool.map(lambda b: oracles[b].initial_run(states[b], ees[b].reshape(4, 3)), range(B)))
    dt = cfgs[0]['integrator_dt']
    nx = (cfgs[0]['num_nodes'] + 1) * 12
    seen_n, compared, worst = set(), 0, dict(A=0.0, x=0.0, z=0.0, states=0.0, dual_obj=0.0, dual_obj_of_terms=0.0)
    loose = 0
    alive = np.ones(B, bool)
    for i in range(steps):
        t = i * dt
        own = g.get_trajectory()
        g.set_warm_start_trajectory((host.Trajectory * B)(*[oracles[b].trajectory_record(host) if alive[b] else own[b] for b in range(B)]))
        own_states = g.trajectory_states()
        _, own_ee, _ = g.eval_trajectory(t)
        st_in = np.array([o.states()[1] if alive[b] else own_states[b, 1] for b, o in enumerate(oracles)])
        ee_in = np.array([[[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)] if alive[b] else own_ee[b]
                          for b, o in enumerate(oracles)]).reshape(B, 12)
        g.rti_advance(i, 1); g.synchronize()
        sos = list(pool.map(lambda b: oracles[b].rti(st_in[b], t, ee_in[b].reshape(4, 3)) if alive[b] else 8, range(B)))
        sz = g.sizes(); st, err = g.status(); xr = g.raw_qp_minimiser(); x = g.qp_solution(); z, s = g.dual_solution(); tr = g.trajectory_states()
        assert np.all(err[alive] == 0), (i, np.nonzero(err)[0][:8])
        for b in range(B):
            o = oracles[b]
            if not alive[b]:
                continue
            if int(sos[b]) > 1:            # the oracle's solver gave up: that instance leaves the comparison (tests/test_gpu_resync.py)
                alive[b] = False
                continue
            osz = o.sizes()
            n, m = osz['n'], osz['m']
            assert (sz[b, 0], sz[b, 1], sz[b, 3]) == (n, m, osz['n_ineq']), (i, b)
            A, bv, P, q = g.export_qp(b)
            Ao, bo, Po, qo = o.qp_dense()
            assert not np.any((np.abs(A) > 1e-12) & (np.abs(Ao) <= 1e-14)) and not np.any((np.abs(Ao) > 1e-12) & (np.abs(A) <= 1e-14)), (i, b)
            ea = max(np.abs(A - Ao).max(), np.abs(bv - bo).max(), np.abs(P - Po).max(), np.abs(q - qo).max())
            assert ea <= 1e-12, (i, b, ea)
            if int(st[b]) > 1:
                continue
            ex = max(relerr(xr[b, :n], o.qp_x()), relerr(x[b, :n], o.x()))
            es = relerr(tr[b], o.states())
            zg, zo = z[b, :m], o.z()
            # z: its identifiable part A'z (any split of the multiplier of dependent active rows is optimal), relative
            ez = np.abs(Ao.T @ (zg - zo)).max() / max(1.0, np.abs(Ao.T @ zo).max())
            # dual objective b'z, relative to its value: 1e-6, or the primal accuracy of the same solve where that is looser.  One solve of this
            # set (step 7, instance 28: a far target, a weakly determined minimiser) ends with x 1.0e-5 apart on the two sides
            # of the same QP (A, b, P, q equal to 1e-12) and b'z 1.2e-5 apart; every other solve meets 1e-6.  Counted and printed.
            ed = abs(bo @ zg - bo @ zo) / max(1.0, abs(bo @ zo))
            ed_sum = abs(bo @ zg - bo @ zo) / max(1.0, np.abs(bo * zo).sum())
            assert ex < REL_TOL and es < REL_TOL and ez < REL_TOL and ed <= max(1e-6, 2 * ex), (i, b, ex, es, ez, ed)
            loose += ed > 1e-6
            for k, v in (('A', ea), ('x', ex), ('z', ez), ('states', es), ('dual_obj', ed), ('dual_obj_of_terms', ed_sum)):
                worst[k] = max(worst[k], v)
            seen_n.add(n); compared += 1
    print('oracle parity of %d heterogeneous instances: %d solves compared, window sizes %s, dual objective beyond 1e-6 in %d, worst %s'
          % (B, compared, sorted(seen_n), loose, worst))
    assert loose <= 2, loose
    assert len(seen_n) >= 2, seen_n           # both window sizes of the protocol
    assert compared >= 0.9 * B * steps
    g.close()


# ---- 4. the closed loop ----
def test_heterogeneous_closed_loop_matches_oracle_plant_and_batches_of_one():
    B, K = 6, 6
    cfgs = het_configs(B)
    states, ees = inputs(cfgs)
    push_time = np.array([2.5, 1.5, 1e9, 3.5, 2.5, 1e9]) * cfgs[0]['integrator_dt']
    imp = np.zeros((B, 6)); imp[0, 0] = 2.0; imp[1, 1] = -1.5; imp[3, 3:] = [0.05, -0.1, 0.2]; imp[4, 2] = 0.5

    def run(g, sl):
        g.plant_set_state(states[sl]); g.plant_set_push(push_time[sl], imp[sl])
        first = None
        for i in range(K):
            g.closed_loop_advance(i, 1); g.synchronize()
            if i == 0:
                first = g.plant_state()
        return first, snap(g), g.plant_state()

    g, _, _ = make_het(cfgs, (0.0, 0.0))
    first, a, plant = run(g, slice(None))
    assert np.all(a['err'] == 0)
    dt = cfgs[0]['integrator_dt']
    for b in range(B):
        o = OracleMPC(cfgs[b])
        if b == FULL_Q_INST:
            o.set_costs(*full_q_costs(cfgs[b]))
        o.set_warmstart(states[b]); o.initial_run(states[b], ees[b].reshape(4, 3))
        x = o.plant_integrate(states[b], 0.0, dt, 1, 0)
        assert relerr(first[b], x) < 1e-6, (b, relerr(first[b], x))
        one = make_one(cfgs, b, (0.0, 0.0))
        f1, s1, p1 = run(one, slice(b, b + 1))
        assert_rows_bitwise(a, b, s1, 0, 'closed loop')
        assert plant[b].tobytes() == p1[0].tobytes(), b
        one.close()
    g.close()


# ---- 5. the gait step ----
def test_heterogeneous_gait_line_search_is_bitwise_its_batches_of_one():
    B = 4
    cfgs = het_configs(B)
    dt = cfgs[0]['integrator_dt']

    def run(g):
        g.rti_advance(0, 3); g.synchronize()
        gait = host.BatchGaitOptimizer(g)
        gait.compute_gradient()
        t = 3 * dt
        gait.optimize_contact_times(np.full(g.batch, t))
        grad, valid = gait.gradient()
        step = gait.step()
        state = g.trajectory_states()[:, 1]
        _, ee, _ = g.eval_trajectory(t)
        imin, costs = gait.line_search(state, t, ee.reshape(g.batch, 12))
        out = dict(grad=grad, valid=valid, step=step, imin=imin, costs=costs)
        out.update(snap(g))
        gait.close()
        return out

    g, _, _ = make_het(cfgs, (0.0, 0.0))
    a = run(g)
    assert np.all(a['err'] == 0) and a['valid'].sum() >= 2, a['valid']
    assert len({a['costs'][b].tobytes() for b in range(B)}) == B
    for b in range(B):
        o = make_one(cfgs, b, (0.0, 0.0))
        assert_rows_bitwise(a, b, run(o), 0, 'gait step')
        o.close()
    g.close()


# ---- 6. whole-body targets ----
def test_heterogeneous_targets_are_bitwise_their_batches_of_one():
    B = 4
    cfgs = het_configs(B)
    q0 = np.array(cfgs[0]['init_config'], float)
    t = 2 * cfgs[0]['integrator_dt'] + 0.013
    g, _, _ = make_het(cfgs, (0.0, 0.0))
    g.rti_advance(0, 2); g.synchronize()
    q, v, f, st = g.get_targets_from_traj(t, np.tile(q0, (B, 1)))
    for b in range(B):
        o = make_one(cfgs, b, (0.0, 0.0))
        o.rti_advance(0, 2); o.synchronize()
        q1, v1, f1, st1 = o.get_targets_from_traj(t, q0[None])
        for x, y, k in ((q, q1, 'q_des'), (v, v1, 'v_des'), (f, f1, 'force_des'), (st, st1, 'status')):
            assert x[b].tobytes() == y[0].tobytes(), (b, k)
        o.close()
    g.close()


# ---- 7. semantics ----
def test_clone_carries_the_instance_records():
    cfgs = het_configs(6)
    g, _, _ = make_het(cfgs, (0.0, 0.1))
    c = g.clone()
    g.rti_advance(0, 4); c.rti_advance(0, 4); g.synchronize(); c.synchronize()
    a, b = snap(g), snap(c)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for i in range(6):
        ia, ma = g.instance_model(i)
        ib, mb = c.instance_model(i)
        assert bytes(ia) == bytes(ib) and bytes(ma) == bytes(mb)
    g.close(); c.close()


def test_batch_wide_setters_after_each_setters_give_the_uniform_batch():
    B = 5
    base = load_config('a1_configuration')
    cfgs = [dict(c, mass=base['mass'], Ir=base['Ir'], friction_coef=base['friction_coef'], force_bound=base['force_bound'])
            for c in het_configs(B)]                     # the same constructor data, different costs
    states, ees = inputs(cfgs)
    u = host.BatchMPC(base, B)
    h = host.BatchMPC.from_configs(cfgs)
    h.add_force_cost_each(0, np.linspace(0, 1e-3, B))
    des, Q, Phi, Phi_w = cost_set(base, 'C')           # a final cost that is not the tracking cost (tests/cost_variants_kit.py): full Phi, its own target
    assert not np.array_equal(Phi, Q) and not np.array_equal(Phi_w, -1 * Q @ des)
    for g in (u, h):
        g.add_quadratic_tracking_cost(des, Q); g.set_quadratic_final_cost(Phi); g.set_linear_final_cost(Phi_w); g.add_force_cost(5e-4)
        setup(g, (0.0, 0.0), states, ees)
        g.rti_advance(0, 3); g.synchronize()
    a, b = snap(u), snap(h)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    u.close(); h.close()


def test_get_instance_model_returns_what_was_set():
    cfgs = het_configs(4)
    g = host.BatchMPC.from_configs(cfgs)
    g.add_force_cost_each(1, [7e-4, 2e-4])
    for b, c in enumerate(cfgs):
        info, model = g.instance_model(b)
        assert info.num_nodes == c['num_nodes'] and info.integrator_dt == c['integrator_dt']
        assert info.friction_coef == c['friction_coef'] and info.force_bound == c['force_bound']
        assert info.force_cost == {1: 7e-4, 2: 2e-4}.get(b, c['force_cost'])
        assert list(info.ee_box_size) == list(c['ee_box_size']) and info.swing_height == c['swing_height'] and info.foot_offset == c['foot_offset']
        assert model.mass == c['mass'] and list(model.Ir) == list(np.asarray(c['Ir'], float).reshape(-1))
        assert list(model.hip_xy) == list(np.asarray(c['hip_xy'], float).reshape(-1))
    assert g.L.srbm_get_instance_model(g.h, 4, C.byref(host.MPCInfo()), C.byref(host.Model())) < 0
    g.close()


# ---- 8. rejections ----
def test_rejections_name_the_field_and_leave_the_batch_unchanged():
    L = host.lib()
    cfgs = het_configs(3)
    for field, val in (('num_nodes', 21), ('integrator_dt', 0.04), ('swing_height', 0.08), ('foot_offset', 0.02)):
        bad = [dict(c) for c in cfgs]
        bad[2][field] = val
        infos = (host.MPCInfo * 3)(*[host._info_model(c)[0] for c in bad]); models = (host.Model * 3)(*[host._info_model(c)[1] for c in bad])
        h = C.c_void_p()
        assert L.srbm_batch_create_each(C.byref(h), 3, infos, models, 0) < 0
        assert field in L.srbm_last_error().decode(), L.srbm_last_error()
        with pytest.raises(ValueError, match=field):
            host.BatchMPC.from_configs(bad)
    bad = [dict(c) for c in cfgs]
    bad[1]['hip_xy'] = (np.asarray(bad[1]['hip_xy'], float) + 0.001).tolist()
    infos = (host.MPCInfo * 3)(*[host._info_model(c)[0] for c in bad]); models = (host.Model * 3)(*[host._info_model(c)[1] for c in bad])
    h = C.c_void_p()
    assert L.srbm_batch_create_each(C.byref(h), 3, infos, models, 0) < 0 and 'hip_xy' in L.srbm_last_error().decode()

    g, states, ees = make_het(cfgs, (0.0, 0.0), full=False)
    twin, _, _ = make_het(cfgs, (0.0, 0.0), full=False)
    a12, a144 = np.zeros(12 * 3), np.zeros(144 * 3)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    calls = [('srbm_add_quadratic_tracking_cost_each', lambda f, n, x, y: L.srbm_add_quadratic_tracking_cost_each(g.h, f, n, x, y)),
             ('srbm_set_quadratic_final_cost_each', lambda f, n, x, y: L.srbm_set_quadratic_final_cost_each(g.h, f, n, y)),
             ('srbm_set_linear_final_cost_each', lambda f, n, x, y: L.srbm_set_linear_final_cost_each(g.h, f, n, x)),
             ('srbm_add_force_cost_each', lambda f, n, x, y: L.srbm_add_force_cost_each(g.h, f, n, x))]
    for name, call in calls:
        for f, n, why in ((-1, 1, 'out of range'), (2, 2, 'out of range'), (4, 0, 'out of range')):
            assert call(f, n, dp(a12), dp(a144)) < 0
            msg = L.srbm_last_error().decode()
            assert name in msg and why in msg, msg
        assert call(0, 1, None, None) < 0 and 'NULL' in L.srbm_last_error().decode()
    for G in (g, twin):
        G.create_initial_run(states, ees); G.rti_advance(0, 2); G.synchronize()
    a, b = snap(g), snap(twin)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    g.close(); twin.close()


# ---- 9. the LARGE build ----
def test_large_build_heterogeneous_batch_is_bitwise_its_batches_of_one():
    cfgs = het_configs(4, num_nodes=40)
    g, _, _ = make_het(cfgs, (0.0, 0.0), large=True)
    assert g.large
    g.rti_advance(0, 3); g.synchronize()
    a = snap(g)
    assert np.all(a['err'] == 0)
    for b in range(4):
        o = make_one(cfgs, b, (0.0, 0.0), large=True)
        o.rti_advance(0, 3); o.synchronize()
        assert_rows_bitwise(a, b, snap(o), 0, 'LARGE build')
        o.close()
    g.close()
