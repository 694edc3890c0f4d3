"""The ground of the torque-driven whole-body plant without a GPU: the numpy restatement of tests/wb_ground_plant_kit.py on its own -- the contact
law holds what it is; the inputs of the GPU tests (test_gpu_wb_ground_plant.py holds the device to 1e-9 on them) sit off every branch point of the
law and take the branches they are meant to take; the drop-and-settle case comes to rest under the kit's ground and actuator values -- with the
names of the tick-log fields of a ground and the decoding of field 63."""
import os
import re

import numpy as np
import pytest

import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_torque_plant_kit as fd
from srbm_loader import host, ROOT
from srbm_loader.controller_rollout import (TICK_LOG_FIELDS, TORQUE_PLANT_LOG_FIELDS, GROUND_PLANT_LOG_FIELDS, GROUND_WORD_OFFSET, decode_ground_word)

MARGIN = 1e-6


@pytest.fixture(scope='module')
def cfg():
    return host.load_config('a1_configuration')


def plant_models(cfg, batch=4):
    """the plant's model per instance of the GPU tests: the controller's bodies on the even instances, bodies of their own on the odd ones"""
    return [kit.Model(fd.plant_cfg(cfg, bodies=fd.perturbed_bodies(cfg, b))) if b % 2 else kit.Model(cfg) for b in range(batch)]


def test_the_restated_law_holds_what_it_is():
    """N >= 0, |T| <= mu N (1 + 1e-12), after a slip the new anchor reproduces T to 1e-12 relative, a first touch sets the anchor at the foot, a foot
    at or above the ground has no force and no state: 4000 seeded feet over every branch"""
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(4000):
        gr = gk.ground_params(rng.normal() * 0.1, k_n=10 ** rng.uniform(2, 5), d_n=10 ** rng.uniform(0, 3) * (rng.random() > 0.1),
                              mu=rng.uniform(0, 1.2) * (rng.random() > 0.1), k_t=10 ** rng.uniform(2, 5), d_t=10 ** rng.uniform(0, 3) * (rng.random() > 0.1))
        p = np.array([rng.normal(), rng.normal(), gr[0] + rng.normal() * 0.01])
        w = rng.normal(size=3) * 10 ** rng.uniform(-2, 1)
        was = rng.random() > 0.4
        cs = np.array([1.0, p[0] + rng.normal() * 10 ** rng.uniform(-5, -1), p[1] + rng.normal() * 10 ** rng.uniform(-5, -1)]) if was else np.zeros(3)
        F, out, info = gk.contact_law(p, w, cs, gr)
        seen.add((info['branch'], info['first']))
        if info['branch'] == gk.AIR:
            assert p[2] >= gr[0] and np.all(F == 0) and np.all(out == 0)
            continue
        assert p[2] < gr[0] and out[0] == 1.0
        assert F[2] >= 0 and (F[2] == 0) == (info['branch'] == gk.CLAMP)
        assert np.hypot(F[0], F[1]) <= gr[3] * F[2] * (1 + 1e-12)
        if info['slip']:
            again = -gr[4] * (p[:2] - out[1:]) - gr[5] * w[:2]
            # (relative to the terms the anchor is formed from: T, d_t w and k_t p_xy -- p_xy - anchor is rounded at the size of p_xy)
            assert np.abs(again - F[:2]).max() <= 1e-12 * max(1.0, np.abs(F[:2]).max(), np.abs(gr[5] * w[:2]).max(), gr[4] * np.abs(p[:2]).max())
        else:
            assert np.array_equal(out[1:], p[:2] if not was else cs[1:])
            assert np.array_equal(F[:2], info['T0'])
    assert seen == {(gk.AIR, False), (gk.STICK, False), (gk.STICK, True), (gk.SLIP, False), (gk.SLIP, True), (gk.CLAMP, False), (gk.CLAMP, True)}
    # the ground never pulls, whatever the foot does; and no ground is no ground
    F, out, _ = gk.contact_law(np.array([0.0, 0.0, -0.01]), np.array([0.0, 0.0, 50.0]), np.zeros(3), gk.ground_params(0.0))
    assert F[2] == 0 and out[0] == 1.0
    F, out, info = gk.contact_law(np.array([0.0, 0.0, -5.0]), np.zeros(3), np.array([1.0, 0.3, 0.2]), gk.ground_params(-np.inf))
    assert info['branch'] == gk.AIR and np.all(F == 0) and np.all(out == 0)


def test_the_gpu_cases_are_off_the_branch_points(cfg):
    """every contact, clamp and stick / slip decision of every GPU case has a margin of 1e-6: |delta|, |k_n delta - d_n w_z|, |n0 - lim| relative to
    max(1, lim).  The solve cases take the branches they name, on feet in different branches within one instance; the step cases, at S = 1 and 3 with
    and without the push, contain the touch-down and the lift-off in sub-step 2, a clamped joint and a zero control action"""
    models = plant_models(cfg)
    worst = np.inf
    seen = set()
    for c in gk.solve_cases(cfg, models):
        for b in range(4):
            _, _, infos = gk.ground_dynamics(models[b], c['q'][b], c['v'][b], c['tau'][b], c['cs'][b], c['ground'][b])
            got = [(i['branch'], i['first']) for i in infos]
            assert got == c['want'][b], (b, got, c['want'][b])
            assert len({g for g in got}) >= 2
            seen |= set(got)
            worst = min(worst, min(min(i['margins']) for i in infos))
    assert seen == {(gk.AIR, False), (gk.STICK, False), (gk.STICK, True), (gk.SLIP, False), (gk.SLIP, True), (gk.CLAMP, False), (gk.CLAMP, True)}
    h = kit.TICK_DT
    ctrl = kit.Model(cfg)
    kp, kd, lim = fd.step_actuators(cfg)
    clamped = off_seen = False
    for c in gk.step_cases(cfg, models, h):
        off = (c['status'][:, 1] & 255) > 1
        for S in (1, 3):
            for b in range(4):
                for push in (None, (c['push_time'][b], c['impulse'][b])):
                    _, _, _, info = gk.ground_step(models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], c['ground'][b],
                                                   h, S, c['k'], ctrl.mass, ctrl.Ir_inv, push)
                    worst = min(worst, min(min(i['margins']) for infos in info['history'] for i in infos))
                    clamped |= info['clamped'] > 0
                    off_seen |= bool(off[b])
                    if S == 3 and b == gk.TOUCH_DOWN[0]:
                        assert [infos[gk.TOUCH_DOWN[1]]['branch'] != gk.AIR for infos in info['history']] == [False, True, True]
                        assert info['history'][1][gk.TOUCH_DOWN[1]]['first']
                    if S == 3 and b == gk.LIFT_OFF[0]:
                        assert [infos[gk.LIFT_OFF[1]]['branch'] != gk.AIR for infos in info['history']] == [True, False, False]
    assert clamped and off_seen
    print('smallest margin over every decision of the GPU cases: %.3g' % worst)
    assert worst >= MARGIN


def test_drop_and_settle_on_the_restatement(cfg):
    """the kit's drop case comes to rest on the restatement: at the end |v|_inf and |sum F_z - m_b g| / (m_b g) are below a tenth of V_REST and
    W_REST, every foot stands and sticks, and the two instances stand on their own grounds"""
    c = gk.settle_case(cfg)
    assert len(c['models']) == 2 and c['weight'][1] > 1.05 * c['weight'][0] and c['ground'][0, 0] != c['ground'][1, 0]
    feet = np.array([kit.ik.forward_kinematics(m.legs, q) for m, q in zip(c['models'], c['q'])])
    assert np.allclose(feet[:, :, 2].min(axis=1) - c['ground'][:, 0], gk.DROP_HEIGHT, rtol=0, atol=1e-12)
    for b, (q, v, cs, sol) in enumerate(gk.settle_restated(cfg)):
        vmax, werr = gk.settle_measures(v, sol, c['weight'][b])
        print('instance %d: |v|_inf %.3g (V_REST %g), weight error %.3g (W_REST %g), base height above the ground %.4f' % (
            b, vmax, gk.V_REST, werr, gk.W_REST, q[2] - c['ground'][b, 0]))
        assert vmax < 0.1 * gk.V_REST and werr < 0.1 * gk.W_REST
        assert np.all(cs[:, 0] == 1) and np.all(sol[18:].reshape(4, 3)[:, 2] > 0)
        assert 0.2 < q[2] - c['ground'][b, 0] < 0.3


def test_the_ground_fields_of_the_tick_log_and_the_decoding_of_field_63():
    text = open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read()
    for field, word in ((60, 'vertical ground force'), (61, 'a_plant'), (62, 'F_ground'), (63, '4096')):
        assert re.search(r'\*\s+%d\s+[^\n]*%s' % (field, re.escape(word)), text), field
    G = GROUND_PLANT_LOG_FIELDS
    assert not set(G) & set(TICK_LOG_FIELDS) and len(G) == 7
    assert (G['plant_kind'], G['clamped_joints'], G['torque_deviation'], G['min_planned_stance_fz'], G['accel_mismatch'], G['force_mismatch'],
            G['ground_word']) == (57, 58, 59, 60, 61, 62, 63)
    assert all(TORQUE_PLANT_LOG_FIELDS[k] == G[k] for k in set(G) & set(TORQUE_PLANT_LOG_FIELDS))
    assert GROUND_WORD_OFFSET == 4096
    d = decode_ground_word(4096.0 + (0b0101 | 0b0100 << 4 | 0b1001 << 8))
    assert d['ground'] and d['in_contact'].tolist() == [True, False, True, False] and d['slipping'].tolist() == [False, False, True, False]
    assert d['plan_differs'].tolist() == [True, False, False, True]
    d = decode_ground_word(np.array([[0.0, 4096.0], [4096.0 + 0xfff, 4097.0]]))
    assert d['ground'].tolist() == [[False, True], [True, True]] and d['in_contact'].shape == (2, 2, 4)
    assert not d['in_contact'][0].any() and d['in_contact'][1, 0].all() and d['slipping'][1, 0].all() and d['plan_differs'][1, 0].all()
    assert d['in_contact'][1, 1].tolist() == [True, False, False, False]
    # the kit's word is the one the decoder reads
    cs = np.array([[1, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0]], float)
    infos = [dict(slip=False), dict(slip=False), dict(slip=True), dict(slip=False)]
    d = decode_ground_word(4096 + gk.ground_word(cs, infos, [1, 1, 0, 1]))
    assert d['in_contact'].tolist() == [True, False, True, True] and d['slipping'].tolist() == [False, False, True, False]
    assert d['plan_differs'].tolist() == [False, True, True, False]
