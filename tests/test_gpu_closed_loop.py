"""Closed-loop rollout harness through the C-ABI: srbm_plant_*, srbm_closed_loop_advance.

The plant is RKIntegrator::CalcIntegral (/root/reference/mpc/rk_integrator.cpp:14-30) over SingleRigidBodyModel::CalcDynamics
(/root/reference/mpc/models/single_rigid_body_model.cpp:222-256) under the forces / foot locations of the current
trajectory; the oracle restates both (oracle/srbm_traj_model.hpp: CalcDynamics, CalcIntegral), tests/closed_loop_kit.py the loop around them
(RestatementLoop).  Tolerances: plant states and trajectories <= 1e-4 relative (the north-star tolerance; a plant step alone agrees to 1e-12)."""
import numpy as np
import pytest

from closed_loop_kit import IMPULSES, NO_GAIT, PUSH_TIMES, RestatementLoop, push_draw
from gpu_kit import REL_TOL, relerr
from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, config_d_instance, instances

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('advance_time', [0, 1])
def test_closed_loop_rollout_matches_oracle(advance_time):
    cfg = load_config()
    B, K, SUB = 3, 6, 5
    states, ees = instances(cfg, config_b_instance, B)
    push_time, impulse = PUSH_TIMES[:B], IMPULSES[:B]             # instance 2 is never pushed
    g = host.BatchMPC.cold_start(cfg, states, ees)
    g.plant_set_state(states); g.plant_set_push(push_time, impulse)
    for i in range(K):                                           # one step per call: the plant state after every step is compared
        g.closed_loop_advance(i, 1, SUB, advance_time); g.synchronize()
        if i == 0: first = g.plant_state()
    st, err = g.status()
    assert np.all(err == 0)
    xs, tr = g.plant_state(), g.trajectory_states()
    for b in range(B):
        loop = RestatementLoop(cfg, states[b], ees[b].reshape(4, 3), NO_GAIT, SUB, advance_time, push_time[b], impulse[b])
        plant = [loop.run()['plant'] for _ in range(K)]
        o = loop.o
        assert relerr(first[b], plant[0]) < 1e-6                 # first plant step: the trajectories of the two cold starts agree to ~1e-6 (observed 8e-8)
        assert relerr(xs[b], plant[-1]) < REL_TOL
        assert relerr(tr[b], o.states()) < REL_TOL
        assert (int(st[b]) in (0, 1, 2)) == (int(o.stats()['status']) in (0, 1, 2))
    # the pushed instances left the unpushed path: the push is visible in the plant momentum
    assert np.abs(xs[0, 3:6] - xs[2, 3:6]).max() > 0.5


def test_closed_loop_fused_steps_equal_single_steps_and_push_distribution():
    """K closed-loop steps in one launch == K launches of one step (bitwise); a Config-D style batch (N = 50, pushes drawn per
    instance) runs without error bits and stays finite"""
    cfg = load_config()
    B, K = 8, 6
    states, ees = instances(cfg, config_b_instance, B)
    pt, imp, rng = push_draw()
    res = []
    for one_launch in (True, False):
        g = host.BatchMPC.cold_start(cfg, states, ees)
        g.plant_set_state(states); g.plant_set_push(pt, imp)
        if one_launch:
            g.closed_loop_advance(0, K, 4, True)
        else:
            for i in range(K): g.closed_loop_advance(i, 1, 4, True)
        g.synchronize()
        res.append((g.plant_state(), g.trajectory_states(), g.qp_solution(), g.status()[0]))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    # without a plant state the entry refuses loudly
    g = host.BatchMPC(cfg, 2)
    with pytest.raises(RuntimeError):
        g.closed_loop_advance(0, 1, 1, False)
    # Config D sizes (its pushes drawn from the same generator, after the eight)
    cfgd = load_config('a1_config_distr_rejection')
    B = 16
    states, ees = instances(cfgd, config_d_instance, B)
    g = host.BatchMPC.cold_start(cfgd, states, ees)
    g.plant_set_state(states)
    g.plant_set_push(rng.uniform(0.0, 0.1, B), rng.normal(0, 1.0, (B, 6)) * np.array([2.5, 2.5, 0.3, 0.1, 0.1, 0.2]))
    g.closed_loop_advance(0, 10, 4, True); g.synchronize()
    st, err = g.status()
    assert np.all(err == 0) and np.all(np.isfinite(g.plant_state())) and np.all(np.isin(st, (0, 1, 2)))
