"""The full MPC update of whole-controller rollouts without a GPU: the four new entries (srbm_controller_set_contact_feedback,
srbm_controller_get_contact_feedback, srbm_controller_contact_feedback_dev, srbm_gait_controller_advance) in the prototype table, in the header
and in the definitions; the methods of ControllerRollout that call them converting under the declared types (the stand-in library of
tests/test_abi_prototypes.py); the refusals that need no device; and the rule of MPC::AdjustForCurrentContacts as tests/contact_feedback_kit.py
restates it for the GPU tests, on a knot table written out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from contact_feedback_kit import classify, posxy, NEAR, GUARD
from srbm_loader import ROOT, controller_rollout, host
from test_abi_prototypes import HANDLE, StandIn

DP = C.POINTER(C.c_double)
ENTRIES = {'srbm_controller_set_contact_feedback': (C.c_int, (C.c_void_p, C.c_int)),
           'srbm_controller_get_contact_feedback': (C.c_int, (C.c_void_p, DP)),
           'srbm_controller_contact_feedback_dev': (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p)),
           'srbm_gait_controller_advance': (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int))}


def test_the_four_entries_are_in_the_table_in_the_header_and_in_the_definitions():
    header = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read(), flags=re.S)
    capi = open(os.path.join(ROOT, 'bilevel-gait-gen_amd', 'csrc', 'srbm_capi.hip')).read()
    for name, proto in ENTRIES.items():
        assert host.PROTOTYPES[name] == proto, name
        assert len(re.findall(r'^int %s\(' % name, header, flags=re.M)) == 1, name
        assert len(re.findall(r'^int %s\(' % name, capi, flags=re.M)) == 1, name
    # the device pointers are those of the one *_dev entry
    assert [n for n, (_, a) in ENTRIES.items() if host.C_TYPES['dev*'] in a[1:]] == ['srbm_controller_contact_feedback_dev']
    # the header cites the lines of the reference each entry replaces, and the kernel file exists under the name the header's section uses
    text = open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read()
    assert 'mpc_controller.cpp:322' in text and 'mpc_controller.cpp:324-346' in text and 'mpc/mpc.cpp:1195-1203' in text
    assert os.path.exists(os.path.join(ROOT, 'bilevel-gait-gen_amd', 'csrc', 'srbm_contact_feedback.hiph'))
    assert controller_rollout.CONTACT_FEEDBACK_DOUBLES == 8


def test_the_methods_convert_under_the_declared_types(monkeypatch):
    fake = StandIn(host.PROTOTYPES, dict(N=50, nu=160, samples=120, knots=32))
    monkeypatch.setitem(host._libs, host.LIB_PATH, fake)
    B = 3
    m = host.BatchMPC(host.load_config('a1_configuration'), B)
    m.h = C.c_void_p(HANDLE)
    go = host.BatchGaitOptimizer(m)
    go.g = C.c_void_p(HANDLE)
    R = controller_rollout.ControllerRollout(m)
    for on in (True, False, 1, 0, np.int64(1)):
        R.set_contact_feedback(on)
    fb = R.contact_feedback()
    assert fb.shape == (B, 4, 2) and fb.dtype == np.float64
    R.contact_feedback_dev(HANDLE, HANDLE + 64)
    R.advance(0, 8, 2, 0.01)
    R.advance(np.int64(20), 8, 2, 1e-2, gait=go, gait_opt_freq=np.int32(3))
    assert set(ENTRIES) | {'srbm_controller_advance'} <= set(fake.calls)
    with pytest.raises(AssertionError, match='srbm_gait_controller_advance: argument 5'):
        R.L.srbm_gait_controller_advance(go.g, 0, 8, 2, 0.01, 2.5)            # (the method converts with int(); the entry itself refuses a float)
    with pytest.raises(AssertionError, match='srbm_controller_contact_feedback_dev: argument 1'):
        R.contact_feedback_dev(np.zeros(B), HANDLE)                             # a host array is not a device address
    # the gait optimiser of another batch, a frequency without an optimiser and an optimiser without a frequency are refused before any call
    n = len(fake.calls)
    other = host.BatchMPC(host.load_config('a1_configuration'), B)
    with pytest.raises(ValueError, match='another batch'):
        controller_rollout.ControllerRollout(other).advance(0, 8, 2, 0.01, gait=go, gait_opt_freq=3)
    with pytest.raises(ValueError, match='gait_opt_freq'):
        R.advance(0, 8, 2, 0.01, gait=go)
    with pytest.raises(ValueError, match='gait_opt_freq'):
        R.advance(0, 8, 2, 0.01, gait_opt_freq=3)
    assert [c for c in fake.calls[n:] if 'advance' in c] == []
    go.close(); m.close(); other.close()


def test_the_refusals_that_need_no_device():
    host.build()
    for L in (host.lib(), host.lib(True)):
        assert L.srbm_controller_set_contact_feedback(None, 1) < 0 and b'srbm_controller_set_contact_feedback' in L.srbm_last_error()
        fb = np.zeros(8)
        assert L.srbm_controller_get_contact_feedback(None, fb.ctypes.data_as(DP)) < 0 and b'srbm_controller_get_contact_feedback' in L.srbm_last_error()
        assert L.srbm_controller_contact_feedback_dev(None, None, None) < 0 and b'srbm_controller_contact_feedback_dev' in L.srbm_last_error()
        assert L.srbm_gait_controller_advance(None, 0, 1, 1, 0.01, 3) < 0
        assert b'srbm_gait_controller_advance' in L.srbm_last_error() and b'NULL handle' in L.srbm_last_error()
        assert L.srbm_controller_advance(None, 0, 1, 1, 0.01) < 0 and b'srbm_controller_advance' in L.srbm_last_error()
        with pytest.raises(C.ArgumentError):
            L.srbm_controller_set_contact_feedback(None, 1.0)
        with pytest.raises(C.ArgumentError):
            L.srbm_controller_get_contact_feedback(None, np.zeros(8, np.int32).ctypes.data_as(C.POINTER(C.c_int)))


def table(times, kinds):
    kn = dict(times=np.zeros((4, 32)), kinds=np.zeros((4, 32), np.int32), nk=np.zeros(4, np.int32))
    for e in range(4):
        kn['nk'][e] = len(times)
        kn['times'][e, :len(times)] = times
        kn['kinds'][e, :len(times)] = kinds
    return kn


def test_the_restated_rule_on_a_knot_table_written_out_by_hand():
    """a foot that swings first: lift-off 0, mid-swing 0.15, touch-down 0.3, two stance-interior knots, lift-off 0.6, mid-swing, touch-down 0.9"""
    kn = table([0.0, 0.15, 0.3, 0.4, 0.5, 0.6, 0.75, 0.9], [0, 3, 1, 2, 2, 0, 3, 1])
    assert posxy(kn, 0)[0].tolist() == [0.0, 0.3, 0.6, 0.9] and posxy(kn, 0)[1].tolist() == [0, 1, 0, 1] and posxy(kn, 0)[2] == [0, 2, 5, 7]
    assert (NEAR, GUARD) == (0.07, 0.1)
    what, away = classify(kn, 0, 0.25)
    assert what == 'moved' and abs(away - 0.05) < 1e-15
    assert classify(kn, 0, 0.22)[0] == 'far' and classify(kn, 0, 0.2300001)[0] == 'moved'
    assert classify(kn, 0, 0.3)[0] == 'held' and classify(kn, 0, 0.45) == ('held', None) and classify(kn, 0, 0.5999)[0] == 'held'
    assert classify(kn, 0, 0.6)[0] == 'far' and classify(kn, 0, 0.85)[0] == 'moved'
    # a foot that stands first: held until its lift-off, then the touch-down that ends that swing
    kn = table([0.0, 0.1, 0.2, 0.3, 0.45, 0.6], [1, 2, 2, 0, 3, 1])
    assert classify(kn, 1, 0.1)[0] == 'held' and classify(kn, 1, 0.3)[0] == 'far' and classify(kn, 1, 0.55)[0] == 'moved'
    with pytest.raises(AssertionError):
        classify(kn, 1, 0.6)                         # the kit's rule is for times inside the table
