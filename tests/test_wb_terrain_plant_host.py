"""The terrain of the torque-driven plant's ground without a GPU: the numpy restatement of tests/wb_terrain_plant_kit.py on its own -- on one
unbounded level patch it returns the bytes of the plane's law; its forces hold what they are on random planes and turn with the scene; the inputs of
the GPU tests (test_gpu_wb_terrain_plant.py holds the device to 1e-9 on them) sit off every branch point and off every patch bound and take the
branches they name; the slope cases meet the kit's thresholds -- with the constants and the prototype of the binding against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_terrain_plant_kit as tk
import wb_torque_plant_kit as fd
from controller_rollout_kit import ik
from srbm_loader import host, ROOT
from srbm_loader import controller_rollout as cr
from test_wb_ground_plant_host import plant_models

MARGIN = 1e-6


@pytest.fixture(scope='module')
def cfg():
    return host.load_config('a1_configuration')


def same(a, b):
    return np.asarray(a, float).tobytes() == np.asarray(b, float).tobytes()


def feet_of(model, q, v):
    p = ik.forward_kinematics(model.legs, q)
    return [(p[i], model.robot.foot_jacobian_lwa(q, i) @ v) for i in range(4)]


# ---- level equals flat ----
def test_on_one_unbounded_level_patch_the_law_returns_the_bytes_of_the_planes_law(cfg):
    """terrain_law against wb_ground_plant_kit.contact_law on every foot of the ground's solve cases and of its step cases (every sub-step of S = 3,
    the contact state carried along): F and the new state byte for byte, the signed zeros included"""
    models = plant_models(cfg)
    feet = branches = 0
    for c in gk.solve_cases(cfg, models):
        for b in range(4):
            level = tk.level_terrain(c['ground'][b])[0]
            for i, (p, w) in enumerate(feet_of(models[b], c['q'][b], c['v'][b])):
                F, out, info = gk.contact_law(p, w, c['cs'][b, i], c['ground'][b])
                Ft, outt, infot = tk.terrain_law(p, w, c['cs'][b, i], c['ground'][b], level)
                assert same(F, Ft) and same(out, outt) and info['branch'] == infot['branch'] and info['first'] == infot['first'], (b, i, F, Ft, out, outt)
                feet += 1; branches += info['branch'] != gk.AIR
    ctrl = kit.Model(cfg)
    kp, kd, lim = fd.step_actuators(cfg)
    for c in gk.step_cases(cfg, models, kit.TICK_DT):
        off = (c['status'][:, 1] & 255) > 1
        for b in range(4):
            level = tk.level_terrain(c['ground'][b])[0]
            a = gk.ground_step(models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], c['ground'][b], kit.TICK_DT, 3, c['k'],
                               ctrl.mass, ctrl.Ir_inv, (c['push_time'][b], c['impulse'][b]))
            t = tk.terrain_step(models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], c['ground'][b], level, kit.TICK_DT, 3,
                                c['k'], ctrl.mass, ctrl.Ir_inv, (c['push_time'][b], c['impulse'][b]))
            for x, y in zip(a[:3], t[:3]):
                assert same(x, y), b
            assert same(a[3]['sol'], t[3]['sol'])
            feet += 12
    # a ground without a plane keeps that switch
    F, out, info = tk.terrain_law(np.array([0.0, 0.0, -5.0]), np.zeros(3), np.array([1.0, 0.3, 0.2]), gk.ground_params(-np.inf), tk.level_terrain(gk.ground_params(0.0))[0])
    assert info['branch'] == tk.AIR and np.all(F == 0) and np.all(out == 0)
    print('%d feet compared, %d of the solve cases in contact' % (feet, branches))
    assert branches >= 16


# ---- force properties ----
def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def test_the_forces_hold_what_they_are_and_turn_with_the_scene():
    """random planes with slopes up to 0.5, 3000 seeded feet over every branch: |T| <= mu N (1 + 1e-12), |T.n| <= 1e-12 max(1, |T|), F.n = N to 1e-12
    (relative to max(1, |F|)); the whole scene turned about the vertical -- the plane, the foot, its velocity, its anchor -- turns F and the new
    anchor with it, to 1e-12 relative to the terms they are formed from (max(1, |F|, (k_n + k_t) |p|, (d_n + d_t) |w|); the anchor: that over k_t)"""
    rng = np.random.default_rng(8)
    seen = set()
    for _ in range(3000):
        gx, gy = rng.uniform(-0.5, 0.5, size=2)
        gr = gk.ground_params(0.0, k_n=10 ** rng.uniform(2, 5), d_n=10 ** rng.uniform(0, 3) * (rng.random() > 0.1), mu=0.0, k_t=10 ** rng.uniform(2, 5),
                              d_t=10 ** rng.uniform(0, 3) * (rng.random() > 0.1))
        mu = rng.uniform(0, 1.2) * (rng.random() > 0.1)
        z0 = rng.normal() * 0.1
        n = np.array(tk.normal(gx, gy))
        xy = rng.normal(size=2)
        p = np.array([xy[0], xy[1], z0 + gx * xy[0] + gy * xy[1] + rng.normal() * 0.01])
        w = rng.normal(size=3) * 10 ** rng.uniform(-2, 1)
        was = rng.random() > 0.4
        cs = np.array([1.0, p[0] + rng.normal() * 10 ** rng.uniform(-5, -2), p[1] + rng.normal() * 10 ** rng.uniform(-5, -2)]) if was else np.zeros(3)
        terrain = tk.patch(z0=z0, gx=gx, gy=gy, mu=mu)
        F, out, info = tk.terrain_law(p, w, cs, gr, terrain)
        seen.add((info['branch'], info['first']))
        # the scene turned by a about the vertical: the gradient turns as a vector
        a = rng.uniform(-np.pi, np.pi)
        Rz = rot_z(a)
        g2 = Rz[:2, :2] @ np.array([gx, gy])
        cs2 = np.concatenate([[cs[0]], Rz[:2, :2] @ cs[1:]]) if was else cs
        F2, out2, info2 = tk.terrain_law(Rz @ p, Rz @ w, cs2, gr, tk.patch(z0=z0, gx=g2[0], gy=g2[1], mu=mu))
        assert info2['branch'] == info['branch'] or min(info['margins'][:3]) < 1e-9
        if info2['branch'] != info['branch']:
            continue
        # (the turned inputs are rounded at the size of p and w, and the law multiplies them by the stiffnesses and dampings: the forces are
        # compared relative to the terms they are formed from, as test_wb_ground_plant_host.py compares the anchor after a slip)
        scale = max(1.0, np.abs(F).max())
        terms = max(scale, (gr[1] + gr[4]) * np.abs(p).max(), (gr[2] + gr[5]) * np.abs(w).max())
        assert np.abs(F2 - Rz @ F).max() <= 1e-12 * terms, (F, F2)
        assert np.abs(out2[1:] - Rz[:2, :2] @ out[1:]).max() <= 1e-12 * max(1.0, np.abs(p).max(), terms / gr[4]) and out2[0] == out[0]
        if info['branch'] == tk.AIR:
            assert np.all(F == 0) and np.all(out == 0)
            continue
        T, N = info['T'], info['N']
        assert N >= 0 and (N == 0) == (info['branch'] == tk.CLAMP) and out[0] == 1.0
        assert np.linalg.norm(T) <= mu * N * (1 + 1e-12)
        assert abs(T @ n) <= 1e-12 * max(1.0, np.linalg.norm(T))
        assert abs(F @ n - N) <= 1e-12 * scale
    assert seen == {(tk.AIR, False), (tk.STICK, False), (tk.STICK, True), (tk.SLIP, False), (tk.SLIP, True), (tk.CLAMP, False), (tk.CLAMP, True)}


# ---- branch margins ----
def test_the_gpu_cases_take_the_branches_they_name_off_every_branch_point_and_patch_bound(cfg):
    """every decision of every seeded GPU input has a margin of 1e-6 -- |delta|, |k_n delta - d_n w_n|, |n0 - lim| relative to max(1, lim) -- and no
    foot is within 1e-6 of a patch bound.  The solve cases take the branch, the (re-)anchoring and the patch SOLVE_FEET names and cover stick, slip
    and clamp on a first touch and with an old anchor, a stored patch that is another one, a foot over no patch, under an overlaid patch, an empty
    patch; the step cases, at S = 1 and 3 with and without the push, contain the touch-down, the lift-off and the slide onto another patch in
    sub-step 2, a clamped joint and a zero control action"""
    models = plant_models(cfg)
    worst = np.inf
    seen = set()
    for c in tk.solve_cases(cfg, models):
        assert c['terrain'].shape == (4, tk.SOLVE_PATCHES, 8)
        for b in range(4):
            _, _, infos = tk.terrain_dynamics(models[b], c['q'][b], c['v'][b], c['tau'][b], c['cs'][b], c['ground'][b], c['terrain'][b])
            got = [(i['branch'], i['first'], i['patch']) for i in infos]
            assert got == c['want'][b], (b, got, c['want'][b])
            assert len({g[0] for g in got}) >= 3 and len({g[2] for g in got}) >= 3
            assert 3 <= sum(pt[0] <= pt[1] for pt in c['terrain'][b]) <= 4 and len({tuple(pt[5:7]) for pt in c['terrain'][b] if pt[0] <= pt[1]}) >= 3
            seen |= {g[:2] for g in got}
            worst = min(worst, min(min(i['margins']) for i in infos))
            # a stored patch that is another one re-anchors
            for i, info in enumerate(infos):
                if info['branch'] != tk.AIR and c['cs'][b, i, 0] not in (0.0, 1.0 + info['patch']):
                    assert info['first']
                    seen.add('other')
    assert seen == {(tk.AIR, False), (tk.STICK, False), (tk.STICK, True), (tk.SLIP, False), (tk.SLIP, True), (tk.CLAMP, False), (tk.CLAMP, True), 'other'}
    wheres = {w for call in tk.SOLVE_FEET for inst in call for w, _, _ in inst}
    assert wheres == {'own', 'over', 'none', 'empty'}
    h = kit.TICK_DT
    ctrl = kit.Model(cfg)
    kp, kd, lim = fd.step_actuators(cfg)
    clamped = off_seen = False
    for c in tk.step_cases(cfg, models, h):
        assert c['terrain'].shape == (4, tk.STEP_PATCHES, 8)
        off = (c['status'][:, 1] & 255) > 1
        for S in (1, 3):
            for b in range(4):
                for push in (None, (c['push_time'][b], c['impulse'][b])):
                    _, _, _, info = tk.terrain_step(models[b], c['q'][b], c['v'][b], c['cs'][b], c['control'][b], off[b], kp[b], kd[b], lim[b], c['ground'][b],
                                                    c['terrain'][b], h, S, c['k'], ctrl.mass, ctrl.Ir_inv, push)
                    worst = min(worst, min(min(i['margins']) for infos in info['history'] for i in infos))
                    clamped |= info['clamped'] > 0
                    off_seen |= bool(off[b])
                    hist = info['history']
                    if S == 3 and b == tk.TOUCH_DOWN[0]:
                        assert [infos[tk.TOUCH_DOWN[1]]['branch'] != tk.AIR for infos in hist] == [False, True, True] and hist[1][tk.TOUCH_DOWN[1]]['first']
                    if S == 3 and b == tk.LIFT_OFF[0]:
                        assert [infos[tk.LIFT_OFF[1]]['branch'] != tk.AIR for infos in hist] == [True, False, False]
                    if S == 3 and b == tk.SLIDE[0]:
                        f = tk.SLIDE[1]
                        assert [infos[f]['patch'] for infos in hist] == [f, 4, 4] and all(infos[f]['branch'] != tk.AIR for infos in hist)
                        assert [infos[f]['first'] for infos in hist] == [False, True, False]
    assert clamped and off_seen
    print('smallest margin over every decision of the GPU cases: %.3g' % worst)
    assert worst >= MARGIN


# ---- the slope cases ----
def test_the_slope_cases_meet_their_thresholds_on_the_restatement(cfg):
    """(a) at rest on the slope under V_REST and W_REST of the ground's kit, every foot sticking; (b) all four feet slipping and the downhill
    acceleration of the base inside the band about g (sin(theta) - mu cos(theta)); the measured values are the ones the kit quotes"""
    c = tk.slope_case(cfg)
    p = ik.forward_kinematics(c['model'].legs, c['q'])
    height = (p - 0.0) @ c['n']                                # the plane passes through the origin
    assert abs(height.min() - gk.DROP_HEIGHT) <= 1e-12 and tk.SLOPE_MU_REST > 2 * np.tan(tk.SLOPE_THETA) > 4 * tk.SLOPE_MU_SLIDE
    v, cs, sol, marks, infos = tk.slope_restated(cfg, 0)
    vmax, werr, _ = tk.slope_measures(v, sol, marks, c)
    print('(a) |v|_inf %.3g (V_REST %g), normal-force error %.3g of the weight (W_REST %g)' % (vmax, gk.V_REST, werr, gk.W_REST))
    assert vmax < gk.V_REST and werr < gk.W_REST
    assert np.all(cs[:, 0] == 1) and all(i['branch'] == tk.STICK for i in infos)
    assert abs(vmax - tk.SLOPE_REST_MEASURED[0]) <= 0.05 * tk.SLOPE_REST_MEASURED[0] and abs(werr - tk.SLOPE_REST_MEASURED[1]) <= 0.05 * tk.SLOPE_REST_MEASURED[1]
    v, cs, sol, marks, infos = tk.slope_restated(cfg, 1)
    _, _, acc = tk.slope_measures(v, sol, marks, c)
    want = tk.slide_closed_form()
    print('(b) downhill acceleration %.4f against %.4f: deviation %.3g (band %g)' % (acc, want, abs(acc - want), tk.SLOPE_SLIDE_BAND))
    assert all(i['branch'] == tk.SLIP for i in infos)
    assert abs(acc - want) <= tk.SLOPE_SLIDE_BAND
    assert abs(abs(acc - want) - tk.SLOPE_SLIDE_MEASURED) <= 0.05 * tk.SLOPE_SLIDE_MEASURED and tk.SLOPE_SLIDE_BAND == 3.0 * tk.SLOPE_SLIDE_MEASURED


# ---- the binding against the header ----
def test_the_constants_and_the_prototype_of_the_binding_are_the_headers(cfg):
    text = open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read()
    assert int(re.search(r'#define SRBM_TERRAIN_PATCHES (\d+)', text).group(1)) == host.TERRAIN_PATCHES == cr.TERRAIN_PATCHES == tk.PATCHES
    assert int(re.search(r'#define SRBM_TERRAIN_DOUBLES (\d+)', text).group(1)) == host.TERRAIN_DOUBLES == cr.TERRAIN_DOUBLES == tk.PATCH_DOUBLES
    assert re.search(r'int srbm_wb_plant_set_terrain\(srbm_batch\* h, const double\* terrain, int n_patches\);', text)
    assert host.PROTOTYPES['srbm_wb_plant_set_terrain'] == (C.c_int, (C.c_void_p, C.POINTER(C.c_double), C.c_int))
    assert same(cr.terrain_patch(x=(0.5, 1.0), z0=0.1, gx=0.2, gy=-0.3, mu=0.4), [0.5, 1.0, -np.inf, np.inf, 0.1, 0.2, -0.3, 0.4])
    assert same(cr.terrain_patch(mu=0.6), tk.patch())
    for word in ('no side faces', 'LAST patch', 'smallest NORMAL'):
        assert word in text, word
