"""The torque-driven whole-body plant without a GPU: the numpy restatement of tests/wb_torque_plant_kit.py on its own -- its (a, F) as the whole-body
dynamics with the stance feet held, for every number of contacts; a body at rest on four feet; the torque law; the sub-steps and the push -- and the
conditioning of the inputs the GPU tests use (test_gpu_wb_torque_plant.py holds the device to 1e-9 on them), with the names of the new tick-log
fields against the header."""
import os
import re

import numpy as np
import pytest

import controller_rollout_kit as kit
import wb_torque_plant_kit as fd
from srbm_loader import host, ROOT
from srbm_loader.controller_rollout import TICK_LOG_FIELDS, TORQUE_PLANT_LOG_FIELDS, FLAG_BREAKDOWN


@pytest.fixture(scope='module')
def cfg():
    return host.load_config('a1_configuration')


def models(cfg):
    """the controller's bodies, and bodies that differ from them"""
    return [kit.Model(cfg), kit.Model(fd.plant_cfg(cfg, bodies=fd.perturbed_bodies(cfg, 1)))]


def test_the_restated_solution_is_the_whole_body_dynamics_with_the_stance_feet_held(cfg):
    """(a, F) of the restatement: kit.dynamics_residual and Js a + Jsdot v within 1e-10 max(1, |tau|_inf), nc = 0 .. 4, both body sets"""
    seen = set()
    for m in models(cfg):
        for q, v, tau, contact in fd.solve_cases(cfg):
            for b in range(len(q)):
                sol = fd.forward_dynamics(m.robot, q[b], v[b], tau[b], contact[b])
                nc = int(contact[b].sum())
                seen.add(nc)
                bound = 1e-10 * max(1.0, np.abs(tau[b]).max())
                res = kit.dynamics_residual(m, q[b], v[b], sol[:18], tau[b], kit.unstack_forces(sol, contact[b]), contact[b])
                assert np.abs(res).max() <= bound, (b, contact[b], np.abs(res).max())
                assert np.all(sol[18 + 3 * nc:] == 0)
                for i in range(4):
                    if contact[b][i]:
                        acc = m.robot.foot_jacobian_lwa(q[b], i) @ sol[:18] + m.robot.foot_classical_acceleration(q[b], v[b], i)
                        assert np.abs(acc).max() <= bound, (b, contact[b], i, np.abs(acc).max())
    assert seen == {0, 1, 2, 3, 4}


def test_a_body_at_rest_on_four_feet_stays_at_rest_under_gravity_compensating_torques(cfg):
    m = kit.Model(cfg)
    q, v, con = np.array(cfg['init_config'], float), np.zeros(18), np.ones(4, int)
    _, _, g = m.robot.dynamics_terms(q, v)
    Js = np.vstack([m.robot.foot_jacobian_lwa(q, i) for i in range(4)])
    F = np.linalg.lstsq(Js.T[:6], g[:6], rcond=None)[0]             # forces that carry the base: 6 rows, 12 unknowns, the smallest ones
    tau = (g - Js.T @ F)[6:]
    sol = fd.forward_dynamics(m.robot, q, v, tau, con)
    assert np.abs(sol[:18]).max() <= 1e-10 and np.abs(sol[18:] - F).max() <= 1e-9
    assert F[2::3].min() > 0 and abs(F[2::3].sum() - m.robot.mass * 9.81) <= 1e-9
    # ... and without the torques it falls: the legs fold under the trunk
    assert fd.forward_dynamics(m.robot, q, v, np.zeros(12), con)[2] < -1.0


def test_the_torque_law(cfg):
    q, v = np.array(cfg['init_config'], float), np.zeros(18)
    ctl = np.concatenate([q[7:] + 0.1, np.full(12, -0.2), np.linspace(-30, 30, 12)])
    lim = np.full(12, 25.0)
    tau, n, dev = fd.torque_law(ctl, q, v, np.full(12, 20.0), np.full(12, 0.5), lim)
    cmd = ctl[24:] + 2.0 - 0.1
    assert np.allclose(tau, np.clip(cmd, -25, 25), rtol=0, atol=1e-13) and n == int((np.abs(cmd) > 25).sum()) and n == 3
    assert dev == np.abs(tau - ctl[24:]).max()
    assert fd.torque_law(ctl, q, v, np.zeros(12), np.zeros(12), np.full(12, np.inf))[:2] == (pytest.approx(ctl[24:], abs=0), 0)
    tau, n, dev = fd.torque_law(np.zeros(36), q, v, np.full(12, 20.0), np.full(12, 0.5), lim, off=True)        # a zero control action: actuators off
    assert np.all(tau == 0) and n == 0 and dev == 0


def test_sub_steps_and_the_push(cfg):
    """one sub-step is the tick-level order of the other plant (velocity, push, configuration); S sub-steps push after the last velocity update; with
    the actuators off the robot falls"""
    m = kit.Model(cfg)
    h = kit.TICK_DT
    c = fd.step_cases(cfg, h)[1]
    kp, kd, lim = fd.step_actuators(cfg)
    b = 2
    assert c['want_push'][b]
    push = (c['push_time'][b], c['impulse'][b])
    args = (m.robot, c['q'][b], c['v'][b], c['control'][b], c['contact'][b], False, kp[b], kd[b], lim[b], h)
    q1, v1, i1 = fd.fd_step(*args, 1, c['k'], m.mass, m.Ir_inv, push)
    tau, _, _ = fd.torque_law(c['control'][b], c['q'][b], c['v'][b], kp[b], kd[b], lim[b])
    a = fd.forward_dynamics(m.robot, c['q'][b], c['v'][b], tau, c['contact'][b])
    qk, vk, pk = kit.plant_step(c['q'][b], c['v'][b], a, h, c['k'], m.mass, m.Ir_inv, False, push)
    assert i1['pushed'] and pk and np.array_equal(q1, qk) and np.array_equal(v1, vk)
    q3, v3, i3 = fd.fd_step(*args, 3, c['k'], m.mass, m.Ir_inv, push)
    q3n, v3n, _ = fd.fd_step(*args, 3, c['k'], m.mass, m.Ir_inv, None)
    assert i3['pushed'] and np.abs(v3[:3] - v3n[:3] - push[1][:3] / m.mass).max() <= 1e-15 and np.array_equal(v3[6:], v3n[6:])
    assert np.abs(q3 - q1).max() > 0                              # the sub-steps move the result
    off = fd.fd_step(m.robot, c['q'][b], np.zeros(18), np.zeros(36), np.ones(4, int), True, kp[b], kd[b], lim[b], h, 2, 0, m.mass, m.Ir_inv)
    assert np.all(off[2]['tau'] == 0) and off[1][2] < -0.01


def test_the_inputs_of_the_gpu_tests_are_well_conditioned(cfg):
    """cond(K) < 1e5 on the inputs of the solve-alone and plant-step GPU tests (every sub-step of the restated step), for both body sets: what lets
    the device be held to 1e-9"""
    worst = 0.0
    for m in models(cfg):
        for q, v, tau, contact in fd.solve_cases(cfg):
            for b in range(len(q)):
                worst = max(worst, np.linalg.cond(fd.kkt_system(m.robot, q[b], v[b], tau[b], contact[b])[0]))
    m = kit.Model(cfg)
    kp, kd, lim = fd.step_actuators(cfg)
    for c in fd.step_cases(cfg, kit.TICK_DT):
        for b in range(len(c['q'])):
            q, v = c['q'][b], c['v'][b]
            for s in range(3):
                tau = fd.torque_law(c['control'][b], q, v, kp[b], kd[b], lim[b], (c['status'][b, 1] & 255) > 1)[0]
                worst = max(worst, np.linalg.cond(fd.kkt_system(m.robot, q, v, tau, c['contact'][b])[0]))
                q, v, _ = fd.fd_step(m.robot, q, v, c['control'][b], c['contact'][b], (c['status'][b, 1] & 255) > 1, kp[b], kd[b], lim[b],
                                     kit.TICK_DT / 3, 1, 0, m.mass, m.Ir_inv)
    print('worst cond(K) over the inputs of the GPU tests: %.3g' % worst)
    assert worst < 1e5


def test_the_new_tick_log_fields_are_the_headers():
    text = open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read()
    for field, word in ((57, 'plant kind'), (58, 'clamped'), (59, 'tau_ff'), (60, 'vertical plant force'), (61, 'a_plant'), (62, 'F_plant')):
        assert re.search(r'\*\s+%d\s+[^\n]*%s' % (field, re.escape(word)), text), field
    F = TORQUE_PLANT_LOG_FIELDS
    assert not set(F) & set(TICK_LOG_FIELDS) and len(F) == 6
    assert (F['plant_kind'], F['clamped_joints'], F['torque_deviation'], F['min_stance_fz'], F['accel_mismatch'], F['force_mismatch']) == (57, 58, 59, 60, 61, 62)
    assert FLAG_BREAKDOWN == 8 and re.search(r'bit 3 a factorisation', text)
