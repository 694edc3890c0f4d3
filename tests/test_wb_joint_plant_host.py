"""The joint model of the torque-driven plant without a GPU (include/srbm_rti.h, "a joint model"; csrc/srbm_wb_joints.hiph): the law the kernels
compile (srbm_joint_law_host) against the Python loop of tests/wb_joint_plant_kit.py bit for bit with every branch taken, the refusals of a setting
(through the host entry, which validates as srbm_wb_plant_set_joints does), the A1 fixture and its mapping by name, the sizes the header states, and
the limp drop on the restatement with the constants the GPU test uses."""
import re
import os

import numpy as np
import pytest

import wb_joint_plant_kit as jk
from gpu_kit import same_bytes
from srbm_loader import host
from srbm_loader import joints as jm
from srbm_loader import controller_rollout as cr


@pytest.fixture(scope='module')
def L():
    return host.lib()


def test_the_law_equals_the_loop_written_from_the_header_bit_for_bit(L):
    """the 12 joints of instance 0 in the 12 branch sets of BRANCH_TABLE in every sub-step, the transparent model, an "off" instance that decays
    through its lags; torque, motor state and record equal bit for bit; the smallest distance of any input to a branch boundary is reported and is
    >= 1e-6"""
    c = jk.law_cases()
    tau_w, js_w, jrec_w, margin, seen = jk.law_restated(c)
    print('smallest distance of an input to a branch boundary: %.3g' % margin)
    assert margin >= jk.MARGIN
    for b in range(3):
        for s in range(jk.LAW_S):
            assert seen[b][s] == c['want'][b], (b, s, seen[b][s])
    flat = {x for br in jk.BRANCH_TABLE for x in br}
    assert flat == {'lag', 'damped', 'band', 'sat+', 'sat-', 'lower', 'lower-clamped', 'upper', 'upper-clamped'} and [] in jk.BRANCH_TABLE
    tau, js, jrec = jm.law(L, jk.LAW_H, c['joints'], c['stops'], c['cmd'], c['off'], c['q_j'], c['v_j'], c['js'])
    same_bytes(tau, tau_w, 'the joint torques')
    same_bytes(js, js_w, 'the motor torques')
    same_bytes(jrec, jrec_w, 'the record')
    # the transparent model returns the command's bytes and keeps no lag; the record counts
    same_bytes(tau[:, 1], c['cmd'][:, 1], 'transparent: t is cmd')
    assert np.all(jrec[1, 1:] == 0) and jrec[1, 0] == jk.LAW_S
    assert jrec[0, 0] == jk.LAW_S and jrec[0, 1] == jk.LAW_S and jrec[0, 5] == float(0b100000011110) and jrec[0, 2] > 0 and jrec[0, 3] > 0 and jrec[0, 4] > 0
    # "off": the lagged motors decay towards 0, the others drop to it at once
    lagged = c['joints'][2][:, jk.JT] > 0
    assert np.all(js[2][~lagged] == 0) and np.all(np.abs(js[2][lagged]) < np.abs(c['js'][2][lagged])) and np.all(js[2][lagged] != 0)
    # a second call continues the first: state and record are carried
    tau2, js2, jrec2 = jm.law(L, jk.LAW_H, c['joints'], c['stops'], c['cmd'], c['off'], c['q_j'], c['v_j'], js, jrec)
    assert jrec2[0, 0] == 2 * jk.LAW_S and np.all(jrec2[:, 2:5] >= jrec[:, 2:5]) and not np.array_equal(js2[0], js[0])


def refusal_cases():
    J, S = np.tile(jk.joint(b=1.0, ia=0.01, fc=0.2, vs=0.1, q_min=-1.0, q_max=1.0, T=1e-3), (3, 12, 1)), np.tile([100.0, 1.0], (3, 1))

    def ch(idx, value, stops=False):
        a, s = J.copy(), S.copy()
        (s if stops else a)[idx] = value
        return a, s
    return [(ch((2, 0, 0), np.nan), 'instance 2, joint 0, field 0'), (ch((1, 4, 0), -0.5), 'instance 1, joint 4, field 0'),
            (ch((0, 11, 1), -1e-3), 'instance 0, joint 11, field 1'), (ch((1, 2, 1), np.inf), 'instance 1, joint 2, field 1'),
            (ch((2, 7, 2), -0.1), 'instance 2, joint 7, field 2'), (ch((0, 3, 3), 0.0), 'instance 0, joint 3, field 3'),
            (ch((0, 5, 2), 0.0), 'instance 0, joint 5, field 3'),                    # f_c = 0 with a band: the band must be 0
            (ch((1, 9, 3), -0.1), 'instance 1, joint 9, field 3'), (ch((2, 1, 4), np.inf), 'instance 2, joint 1, field 4'),
            (ch((0, 6, 4), np.nan), 'instance 0, joint 6, field 4'), (ch((1, 8, 5), -np.inf), 'instance 1, joint 8, field 5'),
            (ch((2, 10, 5), -1.0), 'instance 2, joint 10, field 5'), (ch((0, 0, 6), -1e-3), 'instance 0, joint 0, field 6'),
            (ch((1, 1, 6), np.inf), 'instance 1, joint 1, field 6'), (ch((2, 2, 7), 1.0), 'instance 2, joint 2, field 7'),
            (ch((0, 4, 7), -0.0), 'instance 0, joint 4, field 7'), (ch((1, 0), 0.0, True), 'instance 1, stops, field 0'),
            (ch((2, 0), np.inf, True), 'instance 2, stops, field 0'), (ch((0, 1), -1.0, True), 'instance 0, stops, field 1'),
            (ch((1, 1), np.nan, True), 'instance 1, stops, field 1')]


def test_every_refusal_names_instance_joint_and_field(L):
    z = np.zeros((1, 3, 12))
    for (J, S), msg in refusal_cases():
        with pytest.raises(RuntimeError, match=msg):
            jm.law(L, 1e-3, J, S, z, np.zeros(3, np.int32), z, z, np.zeros((3, 12)))
    # the two allowed infinities, zeros everywhere else
    jm.law(L, 1e-3, jk.transparent(3), np.tile([1.0, 0.0], (3, 1)), z, np.zeros(3, np.int32), z, z, np.zeros((3, 12)))
    for bad in (dict(h=0.0), dict(h=np.nan)):
        with pytest.raises(RuntimeError, match='finite h > 0'):
            jm.law(L, bad['h'], jk.transparent(3), np.tile([1.0, 0.0], (3, 1)), z, np.zeros(3, np.int32), z, z, np.zeros((3, 12)))


def test_the_fixture_loads_and_maps_all_twelve_joints_by_name():
    fx = jk.load_fixture()
    assert len(fx['joints']) == 12 and set(fx['joints']) == set(jm.JOINT_NAMES) and fx['library_order'] == jm.JOINT_NAMES
    assert [n[:2] for n in fx['xml_order'][::3]] == ['FR', 'FL', 'RR', 'RL'] and [n[:2] for n in jm.JOINT_NAMES[::3]] == ['FL', 'FR', 'RL', 'RR']
    cfg = host.load_config('a1_configuration')
    assert [f[:2] for f in cfg['collision_frames']] == ['FL', 'FR', 'RL', 'RR']          # the library's foot order is its joint order
    J, lim = jm.a1_model(fx, 0.1, 2e-3)
    assert J.shape == (12, 8) and np.all(lim == 33.5)
    for i, name in enumerate(jm.JOINT_NAMES):
        part = name.split('_')[1]
        assert J[i, jk.JB] == (2.0 if part == 'hip' else 1.0) and J[i, jk.JIA] == 0.01 and J[i, jk.JFC] == 0.2 and J[i, jk.JVS] == 0.1 and J[i, jk.JT] == 2e-3
        assert (J[i, jk.JQMIN], J[i, jk.JQMAX]) == {'hip': (-0.802851, 0.802851), 'thigh': (-1.0472, 4.18879), 'calf': (-2.69653, -0.916298)}[part]
        assert J[i, 7] == 0
    # a leg swap would show: the fixture with one leg's calf range changed lands on that leg's calf only
    fx['joints']['RL_calf_joint']['range'] = [-2.0, -1.0]
    J2, _ = jm.a1_model(fx, 0.1)
    assert np.flatnonzero(np.any(J2[:, 4:6] != J[:, 4:6], axis=1)).tolist() == [8]
    q0 = np.array(cfg['init_config'], float)[7:]
    assert np.all(q0 > J[:, jk.JQMIN]) and np.all(q0 < J[:, jk.JQMAX])          # the standing pose is inside the ranges
    assert np.array_equal(jm.record(), jk.joint()) and np.array_equal(jm.transparent(), jk.transparent())


def test_the_sizes_are_the_headers():
    text = open(os.path.join(jk.kit.ROOT, 'include', 'srbm_rti.h')).read()
    sizes = {k: int(v) for k, v in re.findall(r'#define (SRBM_JOINT\w+) (\d+)', text)}
    assert sizes == dict(SRBM_JOINT_DOUBLES=8, SRBM_JOINT_STOP_DOUBLES=2, SRBM_JOINT_RECORD_DOUBLES=8)
    for mod in (jm, ):
        assert (mod.JOINT_DOUBLES, mod.STOP_DOUBLES, mod.RECORD_DOUBLES) == (8, 2, 8)
    assert (cr.JOINT_DOUBLES, cr.JOINT_STOP_DOUBLES, cr.JOINT_RECORD_DOUBLES) == (host.JOINT_DOUBLES, host.JOINT_STOP_DOUBLES, host.JOINT_RECORD_DOUBLES) == (8, 2, 8)


def test_the_limp_drop_on_the_restatement_is_stable_and_inside_its_constants():
    """the drop of the GPU test on the restatement alone: finite, all four feet on the ground, the four calves on their stops, the record's excursion and the end speed are the kit's
    constants (to 5 %: they are measured values, the GPU test allows twice them)"""
    cfg = host.load_config('a1_configuration')
    r = jk.drop_restated(cfg)
    vend, exc = float(np.abs(r['v']).max()), float(r['jrec'][2])
    print('limp drop: %d ticks, |v|_inf at the end %.4g, largest excursion %.4g rad, joints ever beyond their range mask %d, base height %.4f, feet in contact %s' % (
        jk.DROP_TICKS, vend, exc, int(r['jrec'][5]), r['q'][2], r['cs'][:, 0]))
    assert np.all(np.isfinite(r['q'])) and np.all(np.isfinite(r['v']))
    assert r['jrec'][0] == jk.DROP_TICKS * jk.DROP_S
    assert abs(vend - jk.DROP_V_END) <= 0.05 * jk.DROP_V_END and abs(exc - jk.DROP_EXCURSION) <= 0.05 * jk.DROP_EXCURSION
    assert exc > 0 and exc < 0.2 and vend < 1.0 and int(r['jrec'][5]) == 0b100100100100 and np.all(r['cs'][:, 0] == 1)
