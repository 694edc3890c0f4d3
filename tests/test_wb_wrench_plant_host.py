"""The wrench schedule of the torque-driven plant without a GPU (include/srbm_rti.h, "timed external wrenches"; csrc/srbm_wb_wrench.hiph): the
generalized force of tests/wb_wrench_plant_kit.py against central differences of the body point and the body rotation and against an independent
identity (a weight hung on a body is the gravity term of the body with a point mass), the activity rule the kernels compile
(srbm_wrench_active_host) against the kit's bit for bit with starts and ends on, beside and between the sub-step times, every refusal of a setting
(through the host entry, which validates as srbm_wb_plant_set_wrenches does), and the builders of srbm_loader.wrenches."""
import copy
import os
import re

import numpy as np
import pytest

import wb_wrench_plant_kit as wk
from controller_rollout_kit import ik
from srbm_loader import controller_rollout as cr
from srbm_loader import host
from srbm_loader import wrenches as wm

kit = wk.kit


@pytest.fixture(scope='module')
def L():
    return host.lib()


@pytest.fixture(scope='module')
def cfg():
    return host.load_config('a1_configuration')


def posture(cfg, rng):
    q = np.array(cfg['init_config'], float)
    q[:3] += rng.normal(size=3) * 0.2
    q[7:] += rng.uniform(-0.4, 0.4, 12)
    quat = rng.normal(size=4)
    q[3:7] = quat / np.linalg.norm(quat)
    return q


def test_the_generalized_force_against_central_differences_of_point_and_rotation(cfg):
    """all 13 bodies and both frames, r off the origin, a force and a torque: Q of the kit's analytic Jacobian against Jv' F + Jw' N with Jv, Jw
    from central differences (step 1e-6) of the body point and the body rotation through ik.integrate; bound 1e-6"""
    rng = np.random.default_rng(3)
    robot = kit.Model(cfg).robot
    eps, worst = 1e-6, 0.0
    for body in range(13):
        for frame in (wk.WORLD, wk.BODY):
            q = posture(cfg, rng)
            w = wk.event(0.0, 1.0, body, rng.uniform(-0.15, 0.15, 3), rng.uniform(-40, 40, 3), rng.uniform(-5, 5, 3), frame)
            Q, _ = wk.generalized_force(robot, q, w[None], 1)
            F, N = wk.world_wrench(robot, q, w)
            want = np.zeros(18)
            for j in range(18):
                e = np.zeros(18); e[j] = eps
                pose = []
                for sgn in (1.0, -1.0):
                    R, o = wk.body_pose(robot, ik.integrate(q, sgn * e, 1.0), body)
                    pose.append((R, o + R @ w[4:7]))
                dx = (pose[0][1] - pose[1][1]) / (2 * eps)
                dR = pose[0][0] @ pose[1][0].T                   # I + 2 eps skew(omega)
                om = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / (4 * eps)
                want[j] = dx @ F + om @ N
            err = np.abs(Q - want).max()
            worst = max(worst, err)
            assert err <= 1e-6, (body, frame, err)
            assert np.abs(Q).max() > 1.0
    print('Q against central differences: worst %.3g' % worst)


def with_point_mass(cfg, body, m_p, r):
    """cfg whose body `body` carries a point mass m_p at r (its joint frame): mass, centre of mass and inertia about the new centre"""
    c = dict(cfg)
    c['body_model'] = copy.deepcopy(cfg['body_model'])
    b = c['body_model'][body]
    m, com, I = b['mass'], np.asarray(b['com'], float), np.asarray(b['inertia'], float).reshape(3, 3)
    r = np.asarray(r, float)
    cn = (m * com + m_p * r) / (m + m_p)
    sk = lambda d: ik.skew(d) @ ik.skew(d).T
    b['mass'], b['com'], b['inertia'] = m + m_p, cn.tolist(), (I + m * sk(com - cn) + m_p * sk(r - cn)).tolist()
    return c


def test_a_weight_hung_on_a_body_is_the_gravity_term_of_the_body_with_a_point_mass(cfg):
    """a world force (0, 0, -9.81 m_p) at r on body i gives Q = g(q; plain) - g(q; body i plus a point mass m_p at r), g from Robot.dynamics_terms
    on the modified body_model; bound 1e-10 max(1, |Q|_inf), all 13 bodies"""
    rng = np.random.default_rng(4)
    plain = kit.Model(cfg).robot
    worst = 0.0
    for body in range(13):
        q = posture(cfg, rng)
        m_p, r = rng.uniform(0.5, 3.0), rng.uniform(-0.15, 0.15, 3)
        w = wk.event(0.0, 1.0, body, r, (0.0, 0.0, -9.81 * m_p))
        Q, _ = wk.generalized_force(plain, q, w[None], 1)
        loaded = kit.Model(with_point_mass(cfg, body, m_p, r)).robot
        want = plain.dynamics_terms(q, np.zeros(18))[2] - loaded.dynamics_terms(q, np.zeros(18))[2]
        err = np.abs(Q - want).max() / max(1.0, np.abs(Q).max())
        worst = max(worst, err)
        assert err <= 1e-10, (body, err)
        assert np.abs(Q).max() > 1.0
    print('Q against the gravity term of a point mass: worst %.3g relative' % worst)


def dur(t0, end):
    """d with t0 + d == end in one rounded sum (the rule forms te = t0 + d)"""
    d = np.float64(end) - np.float64(t0)
    for _ in range(8):
        te = np.float64(t0) + d
        if te == end:
            return float(d)
        d = np.nextafter(d, np.inf if te < end else -np.inf)
    raise AssertionError((t0, end))


def boundary_schedule(h, S, k0):
    """windows in mid-rollout whose starts and ends lie on a computed ts exactly, one ulp to either side of it, and strictly between two sub-steps;
    d = 0 and d = +inf -> W[3][8][16] (instance 1 shifted by a tick, instance 2 empty slots and a never-ending event)"""
    ts = lambda k, s: float(wk.substep_time(k, h, S, s))
    up, dn = lambda x: float(np.nextafter(x, np.inf)), lambda x: float(np.nextafter(x, -np.inf))
    hs = h / S
    out = np.zeros((3, 8, 16))
    for b in range(2):
        k = k0 + b
        a, e = ts(k, S - 1), ts(k + 2, 0)
        ev = [wk.event(a, dur(a, e), 0), wk.event(dn(a), dur(dn(a), e), 1), wk.event(up(a), dur(up(a), up(e)), 2), wk.event(a + 0.5 * hs, 2.25 * hs, 3),
              wk.event(a, dur(a, dn(e)), 4), wk.event(a, 0.0, 5), wk.event(ts(k + 1, 0), np.inf, 6), wk.event(ts(k, 0), hs, 7)]
        out[b] = wk.pad(ev, 8)
    out[2] = wk.pad([wk.event(0.0, 0.0, 0), wk.event(ts(k0 + 1, S // 2), np.inf, 12), wk.event(-1.0, 0.5, 3)], 8)
    return out


def test_the_activity_rule_equals_the_kits_bit_for_bit(L):
    """srbm_wrench_active_host against the rule written from the header: tick_dt 1e-3 and 2e-3, S 1 / 3 / 4, windows in mid-rollout"""
    k0, ticks = 37, 6
    for h in (1e-3, 2e-3):
        for S in (1, 3, 4):
            W = boundary_schedule(h, S, k0)
            first = k0 - 2
            got = wm.active(L, W, first, ticks, h, S)
            want = wk.active_masks(W, first, ticks, h, S)
            assert got.shape == (ticks, S, 3) and np.array_equal(got, want), (h, S, got.tolist(), want.tolist())
            seen = np.bitwise_or.reduce(got.reshape(-1, 3), axis=0)
            assert seen[0] == 0b11011111, (h, S, bin(seen[0]))                # every window acts somewhere but the empty slot (event 5)
            assert seen[2] == 0b10, (h, S, bin(seen[2]))                      # d = 0 never, the past event never, d = +inf from its start
            start = (k0 + 1 - first) * S + S // 2
            assert not np.any(got.reshape(-1, 3)[:start, 2]) and np.all(got.reshape(-1, 3)[start:, 2] == 2)
            # exactly on a ts the event is on at its start and off at its end; one ulp decides
            flat = got.reshape(-1, 3)[:, 0]
            ia, ie = (k0 - first) * S + S - 1, (k0 + 2 - first) * S
            assert flat[ia] & 1 and not flat[ie] & 1 and not flat[ia - 1] & 1           # event 0: [a, e)
            assert flat[ia] & 2 and not flat[ie] & 2                                   # event 1 starts an ulp early
            assert not flat[ia] & 4 and flat[ie] & 4 and not flat[ie + 1] & 4          # event 2 starts an ulp late, ends an ulp late
            assert flat[ie - 1] & 16 and not flat[ie] & 16                             # event 4 ends an ulp early
    # the rule needs no GPU and a cut changes nothing: two halves are the whole
    W = boundary_schedule(1e-3, 4, k0)
    whole = wm.active(L, W, k0 - 2, 6, 1e-3, 4)
    assert np.array_equal(np.concatenate([wm.active(L, W, k0 - 2, 2, 1e-3, 4), wm.active(L, W, k0, 4, 1e-3, 4)]), whole)


def refusal_cases():
    W = np.tile(wk.event(0.1, 0.2, 4, (0.1, 0, 0), (1, 2, 3), (0.1, 0.2, 0.3), 1), (3, 2, 1))

    def ch(idx, value):
        a = W.copy()
        a[idx] = value
        return a
    cases = [(ch((2, 0, 0), np.nan), 'instance 2, event 0, field 0'), (ch((1, 1, 0), np.inf), 'instance 1, event 1, field 0'),
             (ch((0, 1, 1), -1e-3), 'instance 0, event 1, field 1'), (ch((1, 0, 1), np.nan), 'instance 1, event 0, field 1'),
             (ch((2, 1, 1), -np.inf), 'instance 2, event 1, field 1'), (ch((0, 0, 2), 13.0), 'instance 0, event 0, field 2'),
             (ch((1, 1, 2), -1.0), 'instance 1, event 1, field 2'), (ch((2, 0, 2), 2.5), 'instance 2, event 0, field 2'),
             (ch((0, 1, 2), np.nan), 'instance 0, event 1, field 2'), (ch((1, 0, 3), 2.0), 'instance 1, event 0, field 3'),
             (ch((2, 1, 3), 0.5), 'instance 2, event 1, field 3'), (ch((0, 0, 3), -1.0), 'instance 0, event 0, field 3')]
    for f in range(4, 13):
        cases.append((ch((f % 3, f % 2, f), np.inf if f % 2 else np.nan), 'instance %d, event %d, field %d' % (f % 3, f % 2, f)))
    for f in (13, 14, 15):
        cases.append((ch((f % 3, 1, f), 1.0 if f != 14 else -0.0), 'instance %d, event 1, field %d' % (f % 3, f)))
    return W, cases


def test_every_refusal_names_instance_event_and_field(L):
    W, cases = refusal_cases()
    assert wm.active(L, W, 0, 1, 1e-3, 1).shape == (1, 1, 3)
    for bad, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            wm.active(L, bad, 0, 1, 1e-3, 1)
    # the one allowed infinity, the empty slot, the two ends of the body range
    ok = W.copy(); ok[0, 0, 1] = np.inf; ok[1, 1, 1] = 0.0; ok[2, 0, 2] = 0.0; ok[2, 1, 2] = 12.0
    wm.active(L, ok, 0, 1, 1e-3, 1)
    for n in (0, 9):
        with pytest.raises(RuntimeError, match='n_events %d' % n):
            wm.active(L, np.zeros((2, n, 16)), 0, 1, 1e-3, 1)
    with pytest.raises(RuntimeError, match='substeps >= 1'):
        wm.active(L, W, 0, 1, 1e-3, 0)
    with pytest.raises(RuntimeError, match='tick_dt > 0'):
        wm.active(L, W, 0, 1, 0.0, 1)


def test_the_builders_and_the_sizes_are_the_headers():
    text = open(os.path.join(kit.ROOT, 'include', 'srbm_rti.h')).read()
    sizes = {k: int(v) for k, v in re.findall(r'#define (SRBM_WRENCH\w+) (\d+)', text)}
    assert sizes == dict(SRBM_WRENCH_EVENTS=8, SRBM_WRENCH_DOUBLES=16, SRBM_WRENCH_RECORD_DOUBLES=8)
    assert (wm.EVENTS, wm.EVENT_DOUBLES, wm.RECORD_DOUBLES) == (cr.WRENCH_EVENTS, cr.WRENCH_DOUBLES, cr.WRENCH_RECORD_DOUBLES) == (8, 16, 8)
    assert wm.BODY_NAMES[0] == 'trunk' and wm.BODY_NAMES[1 + 3 * 2 + 1] == 'RL_thigh' and len(wm.BODY_NAMES) == 13
    e = wm.event(0.5, 0.15, 'FR_calf', point=(0.01, 0.02, -0.1), force=(1, 2, 3), torque=(4, 5, 6), frame='body')
    assert np.array_equal(e, wk.event(0.5, 0.15, 6, (0.01, 0.02, -0.1), (1, 2, 3), (4, 5, 6), wk.BODY))
    assert np.array_equal(wm.event(1.0, np.inf, 0, force=(0, 0, -1)), wk.event(1.0, np.inf, 0, force=(0, 0, -1)))
    W = wm.schedule(3, [[e], [], [e, wm.event(0, 1, 'trunk')]])
    assert W.shape == (3, 2, 16) and np.array_equal(W[0, 0], e) and not W[0, 1].any() and not W[1].any() and W[2, 1, 1] == 1
    assert np.array_equal(wm.schedule(2, [[e]]), np.tile(e, (2, 1, 1))) and wm.schedule(2, [[]]).shape == (2, 1, 16)
    with pytest.raises(ValueError):
        wm.schedule(2, [[e] * 9])
    with pytest.raises(ValueError):
        wm.schedule(3, [[e], [e]])
