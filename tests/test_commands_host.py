"""The command schedule of a whole-controller rollout without a GPU (include/srbm_rti.h, "timed motion commands"; csrc/srbm_command.hiph): the rule
the kernel compiles (srbm_command_target_host) against the plain-Python restatement of tests/command_kit.py, bit for bit on targets, costs, state
and record; a sequence of updates folded in one call against two calls with the carried state and record; every refusal of a schedule (through the
host entry, which validates as srbm_controller_set_commands does); the prototypes, the exported sizes and the builders of srbm_loader.commands."""
import os
import re

import numpy as np
import pytest

import command_kit as cmk
from gpu_kit import same_bytes
from srbm_loader import commands as cm
from srbm_loader import controller_rollout as cr
from srbm_loader import host

B, NU = 5, 7
TIMES = 0.05 * (1 + np.arange(NU))                 # the update times: a period of 50 ms


@pytest.fixture(scope='module')
def L():
    return host.lib()


def inputs():
    Q, Phi = cmk.cost_matrices(B)
    return cmk.host_schedule(B, TIMES), Q, Phi, np.tile(TIMES[:, None], (1, B)), cmk.host_states(NU, B)


def test_the_host_rule_is_the_restatement_bit_for_bit(L):
    """B = 5 instances (the last with a full Q and a full Phi, Phi != Q everywhere), 7 updates, three events per instance: an absolute one that
    begins exactly at an update time (even instances) or strictly between two (odd ones), a relative one with a lead > 0 after it, an absolute one
    again.  The first update lies before every t0: its outputs are NaN and it leaves state and record as they were"""
    cmds, Q, Phi, times, states = inputs()
    assert np.all(cmds[:, 0, 0] > TIMES[0]) and np.all(cmds[::2, 0, 0] == TIMES[1]) and np.all((cmds[1::2, 0, 0] < TIMES[1]))
    assert np.all((cmds[:, 1, 0] > TIMES[2]) & (cmds[:, 1, 0] < TIMES[3])) and np.all(cmds[:, 1, 1] == 1) and np.all(cmds[:, 1, 2] > 0)
    assert np.any(Q[-1].reshape(12, 12)[~np.eye(12, dtype=bool)] != 0) and not np.array_equal(Q, Phi)
    got = cm.targets(L, cmds, Q, Phi, times, states)
    want = cmk.fold(cmds, Q, Phi, times, states)
    for k in ('des12', 'w12', 'Phi_w12', 'cstate', 'crec'):
        same_bytes(got[k], want[k], k)
    # what the restatement says is what the issue says, on the figures themselves
    assert not got['in_force'][0].any() and got['in_force'][1:].all()
    assert np.isnan(got['w12'][0]).all() and np.isnan(got['Phi_w12'][0]).all()
    rec = got['crec']
    assert np.all(rec[:, 0] == NU - 1) and np.all(rec[:, 1] == 2) and np.all(rec[:, 2] == 3) and np.all(rec[:, 3] == TIMES[5])
    assert np.all(rec[:, 4:6] == 0) and np.all(got['cstate'] == np.array([2, 0, 0, TIMES[5]]))          # the last latch is of an absolute event
    assert np.all(rec[:, 6] > 0) and np.all(rec[:, 7] >= rec[:, 6] ** 2) and np.all(rec[:, 20:] == 0)
    same_bytes(rec[:, 8:20], got['des12'][-1], 'the des last written')
    # the relative event: anchored at the state of ITS first update (times[3]), the anchor held at the next although the state has moved
    for b in range(B):
        ev = cmds[b, 1]
        for u in (3, 4):
            s = (TIMES[u] - ev[0]) + ev[2]
            assert got['des12'][u, b, 0] == (ev[4] + ev[16] * s) + states[3, b, 0] and states[4, b, 0] != states[3, b, 0]
            assert got['des12'][u, b, 1] == (ev[5] + ev[17] * s) + states[3, b, 1]
            assert got['des12'][u, b, 2] == ev[6] + ev[18] * s
    # an update before every t0, alone: nothing is touched
    cs0, cr0 = cm.initial_state(B)
    first = cm.targets(L, cmds, Q, Phi, times[:1], states[:1])
    same_bytes(first['cstate'], cs0, 'state'); same_bytes(first['crec'], cr0, 'record')
    assert np.isnan(first['des12']).all()
    # w of a diagonal Q is -Q_ii des_i, and the sum order of the full one is the setter's (j ascending, separately rounded)
    d = got['des12'][2, 0]
    same_bytes(got['w12'][2, 0], -1 * np.diag(Q[0].reshape(12, 12)) * d, 'diagonal')
    a = np.float64(0)
    for j in range(12):
        a = a + Q[-1][12 * 3 + j] * got['des12'][2, -1, j]
    assert got['w12'][2, -1, 3] == -1 * a


def test_seven_updates_in_one_call_are_three_and_four_with_the_carried_state_and_record(L):
    cmds, Q, Phi, times, states = inputs()
    one = cm.targets(L, cmds, Q, Phi, times, states)
    a = cm.targets(L, cmds, Q, Phi, times[:3], states[:3])
    b = cm.targets(L, cmds, Q, Phi, times[3:], states[3:], a['cstate'], a['crec'])
    for k in ('des12', 'w12', 'Phi_w12'):
        same_bytes(np.concatenate([a[k], b[k]]), one[k], k)
    same_bytes(b['cstate'], one['cstate'], 'state'); same_bytes(b['crec'], one['crec'], 'record')
    # a cut after update 3 lies between the relative event's latch and its next update: the anchor is carried by the state
    c = cm.targets(L, cmds, Q, Phi, times[:4], states[:4])
    assert np.all(c['cstate'][:, 0] == 1) and np.array_equal(c['cstate'][:, 1:3], states[3, :, :2]) and np.all(c['cstate'][:, 3] == TIMES[3])
    d = cm.targets(L, cmds, Q, Phi, times[4:], states[4:], c['cstate'], c['crec'])
    same_bytes(np.concatenate([c['des12'], d['des12']]), one['des12'], 'des12: 4 + 3')
    same_bytes(d['cstate'], one['cstate'], 'state: 4 + 3'); same_bytes(d['crec'], one['crec'], 'record: 4 + 3')


def refuse(L, cmds, n=None, match=''):
    c = np.ascontiguousarray(cmds, float)
    Q, Phi = cmk.cost_matrices(B)
    with pytest.raises(RuntimeError, match=match):
        if n is None:
            cm.targets(L, c, Q, Phi, np.zeros((0, B)), np.zeros((0, B, 13)))
        else:
            cs, cr_ = cm.initial_state(B)
            one = np.zeros(1)
            d = lambda a: a.ctypes.data_as(cm._dp)
            if L.srbm_command_target_host(n, d(c), B, d(Q), d(Phi), 0, d(one), d(one), d(cs), d(one), d(one), d(one), d(cr_)) != 0:
                raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
            raise AssertionError('accepted')


def test_every_refusal_names_the_entry_the_instance_the_event_and_the_field(L):
    good = cmk.host_schedule(B, TIMES)
    cm.targets(L, good, *cmk.cost_matrices(B), np.zeros((0, B)), np.zeros((0, B, 13)))          # the schedule itself is accepted
    fn = 'srbm_command_target_host: '
    for n in (-1, 9):
        refuse(L, np.zeros(B * 9 * 28), n, fn + 'n_events %d' % n)
    for bad in (np.nan, np.inf, -np.inf):
        for f in (0, 2, 4, 15, 16, 27):
            c = good.copy(); c[3, 1, f] = bad
            refuse(L, c, match=fn + r'instance 3, event 1, field %d \(.*\): must be finite' % f)
    c = good.copy(); c[2, 2, 0] = c[2, 1, 0]                  # equal is not ascending
    refuse(L, c, match=fn + r'instance 2, event 2, field 0 \(the start t0\): must ascend')
    c = good.copy(); c[0, 1, 0] = c[0, 0, 0] - 0.01
    refuse(L, c, match=fn + r'instance 0, event 1, field 0 \(the start t0\): must ascend')
    for flag in (2.0, 3.0, -1.0, 0.5):
        c = good.copy(); c[4, 0, 1] = flag
        refuse(L, c, match=fn + r'instance 4, event 0, field 1 \(the flags\): must be 0 or 1')
    c = good.copy(); c[1, 2, 2] = -1e-9
    refuse(L, c, match=fn + r'instance 1, event 2, field 2 \(the lead\): must be >= 0')
    for r in (1.0, -0.0, 1e-300):
        c = good.copy(); c[1, 0, 3] = r
        refuse(L, c, match=fn + r'instance 1, event 0, field 3 \(reserved\): must be 0')
    # the set-up entry validates with the same function under its own name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bilevel-gait-gen_amd', 'csrc', 'srbm_capi.hip')).read()
    body = re.search(r'int srbm_controller_set_commands\(.*?\n}\n', src, flags=re.S).group(0)
    assert 'check_commands(fn, B, cmds, n_events)' in body and 'fn = "srbm_controller_set_commands"' in body


def test_the_prototypes_the_exported_sizes_and_the_builders(L):
    names = {'srbm_controller_set_commands', 'srbm_controller_get_commands', 'srbm_controller_get_command_state', 'srbm_controller_set_command_state',
             'srbm_controller_get_command_record', 'srbm_controller_get_command_costs', 'srbm_controller_command_dev', 'srbm_command_target_host',
             'srbm_command_event_doubles', 'srbm_command_record_doubles'}
    assert names <= set(host.PROTOTYPES)
    assert L.srbm_command_event_doubles() == 28 == cm.EVENT_DOUBLES == cr.COMMAND_DOUBLES == cmk.EVENT_DOUBLES
    assert L.srbm_command_record_doubles() == 32 == cm.RECORD_DOUBLES == cr.COMMAND_RECORD_DOUBLES == cmk.REC_DOUBLES
    assert host.lib(True).srbm_command_event_doubles() == 28 and host.lib(True).srbm_command_record_doubles() == 32
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'srbm_rti.h')).read()
    for k, v in (('SRBM_CMD_MAX_EVENTS', 8), ('SRBM_CMD_EVENT_DOUBLES', 28), ('SRBM_CMD_STATE_DOUBLES', 4), ('SRBM_CMD_REC_DOUBLES', 32)):
        assert re.search(r'#define %s %d\n' % (k, v), hdr), k
    des = np.arange(1.0, 13.0)
    h = cm.hold(0.25, des)
    assert h.shape == (28,) and h[0] == 0.25 and not h[1:4].any() and np.array_equal(h[4:16], des) and not h[16:].any()
    w = cm.walk(0.5, 0.3, -0.1, 12.5, des, lead=0.05)
    want = des.copy(); want[3], want[4] = 12.5 * 0.3, 12.5 * -0.1
    assert w[0] == 0.5 and w[1] == 1 and w[2] == 0.05 and w[3] == 0 and np.array_equal(w[4:16], want)
    assert w[16] == 0.3 and w[17] == -0.1 and not w[18:].any()
    assert cm.walk(0.5, 0.3, 0.0, 12.5, des, relative=False)[1] == 0
    same_bytes(h, cmk.event(0.25, des), 'the kit builds the same event')
    s = cm.stack([[h, w]], batch=3)
    assert s.shape == (3, 2, 28) and np.array_equal(s[2, 1], w)
    s = cm.stack([[h], [w]])
    assert s.shape == (2, 1, 28) and np.array_equal(s[1, 0], w)
    with pytest.raises(ValueError, match='same number'):
        cm.stack([[h], [h, w]])
    with pytest.raises(ValueError, match='at most 8'):
        cm.stack([[h] * 9])
