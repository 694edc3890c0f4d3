"""The control tick without a GPU: the numpy restatements of tests/control_tick_kit.py against a plain loop and a hand-computed case, and the new
entries in the header and in the prototype table of the binding."""
import itertools
import os
import re

import numpy as np

from control_tick_kit import reconstruct_state, stack_forces
from srbm_loader import host, ROOT

ENTRIES = ('srbm_control_tick_reset', 'srbm_control_tick', 'srbm_control_tick_dev')


def test_stacking_for_all_sixteen_contact_patterns():
    """mpc_controller.cpp:181-188 as a loop: force_des.segment<3>(3 j) = GetForce(i) for the j-th foot in contact"""
    pats = np.array(list(itertools.product([0, 1], repeat=4)), np.int32)
    rng = np.random.default_rng(1)
    f = rng.normal(size=(16, 4, 3)) * 50
    out = stack_forces(f, pats)
    assert out.shape == (16, 12)
    for b, con in enumerate(pats):
        want, j = np.zeros(12), 0
        for i in range(4):
            if con[i]:
                want[3 * j:3 * j + 3] = f[b, i]; j += 1
        assert np.array_equal(out[b], want), con          # (-0.0 == 0.0 behind the feet in contact)
    # the flags are only tested for non-zero, as the kernel does
    assert np.array_equal(stack_forces(f[5:6], [[0, 7, 0, 2]]), stack_forces(f[5:6], [[0, 1, 0, 1]]))


def test_reconstruct_state_on_a_hand_computed_case():
    q = np.zeros(19); q[:3] = [1.0, -2.0, 0.5]; q[3:7] = [0.0, 0.0, 0.6, 0.9]          # |quat|^2 = 1.17
    v = np.zeros(18); v[:6] = [0.5, 0.25, -1.0, 2.0, 0.0, -1.0]
    Ir = np.array([[2.0, 0.0, 0.5], [0.0, 3.0, 0.0], [0.5, 0.0, 4.0]])
    s = reconstruct_state(q, v, 4.0, Ir)
    a = (3.0 - 1.17) / 2.0                                                               # first-order normalisation: 0.915
    assert np.array_equal(s[:6], [1.0, -2.0, 0.5, 2.0, 1.0, -4.0])
    assert np.allclose(s[6:10], [0.0, 0.0, 0.6 * a, 0.9 * a], rtol=0, atol=1e-15)
    assert np.array_equal(s[10:], [3.5, 0.0, -3.0])                                      # Ir w, not Ir vel_frame
    # a unit quaternion stays what it is; batches go through unchanged
    q[3:7] = [0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(reconstruct_state(np.tile(q, (3, 1)), np.tile(v, (3, 1)), 4.0, Ir)[2, 6:10], [0.0, 0.0, 0.0, 1.0])


def test_the_entries_are_in_the_header_and_in_the_prototype_table():
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r'^int %s\(srbm_batch\* h,' % name, text, flags=re.M), name
        assert name in host.PROTOTYPES and host.PROTOTYPES[name][0] is host.C_TYPES['int']
    dev, hostp = host.PROTOTYPES['srbm_control_tick_dev'][1], host.PROTOTYPES['srbm_control_tick'][1]
    assert len(dev) == len(hostp) == 12 and all(t is host.C_TYPES['dev*'] for t in dev[1:])
    # status is int[batch][2], contact int[batch][4]; measured contacts are not an argument (one int array in, none)
    assert [i for i, t in enumerate(hostp) if t is host.C_TYPES['int*']] == [6, 9]
