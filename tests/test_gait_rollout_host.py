"""The Python surface of the closed-loop rollout with the gait step (bilevel-gait-gen_amd/gait_rollout.py), no GPU: its three entries in the
prototype table and in the header, every method of GaitRollout converting under the declared types (the stand-in library of
tests/test_abi_prototypes.py), and the decoding of fields 58..63 of a step-log record."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from srbm_loader import ROOT, gait_rollout, host
from test_abi_prototypes import HANDLE, StandIn

ENTRIES = {'srbm_gait_closed_loop_advance': (C.c_int, (C.c_void_p,) + (C.c_int,) * 5),
           'srbm_plant_advance': (C.c_int, (C.c_void_p,) + (C.c_int,) * 3 + (C.POINTER(C.c_double),) * 3),
           'srbm_gait_get_line_search_result': (C.c_int, (C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)))}


def test_the_three_entries_are_in_the_table_and_in_the_header():
    header = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read(), flags=re.S)
    for name, proto in ENTRIES.items():
        assert host.PROTOTYPES[name] == proto, name
        assert len(re.findall(r'^int %s\(' % name, header, flags=re.M)) == 1, name
    # no device-pointer parameters among them
    assert all(a is not host.C_TYPES['dev*'] for _, args in ENTRIES.values() for a in args[1:])


def test_every_method_of_gait_rollout_converts_under_the_declared_types(monkeypatch):
    fake = StandIn(host.PROTOTYPES, dict(N=50, nu=160, samples=120, knots=32))
    monkeypatch.setitem(host._libs, host.LIB_PATH, fake)
    B = 3
    m = host.BatchMPC(host.load_config('a1_configuration'), B)
    m.h = C.c_void_p(HANDLE)
    go = host.BatchGaitOptimizer(m)
    go.g = C.c_void_p(HANDLE)
    r = gait_rollout.GaitRollout(m, go)
    assert r.L is fake
    cases = {'advance': [(1, 11, 5), (np.int64(6), 3, 5, 4, True), (1, 0, 1000, 1, 0)],
             'plant_advance': [(0,), (np.int32(3), 4, True)],
             'line_search_result': [()]}
    assert set(cases) == {n for n, f in inspect.getmembers(gait_rollout.GaitRollout, callable) if not n.startswith('_')}
    for name, argsets in cases.items():
        for args in argsets:
            getattr(r, name)(*args)
    state, time, ee = r.plant_advance(2)
    assert (state.shape, time.shape, ee.shape) == ((B, 13), (B,), (B, 4, 3))
    imin, costs = r.line_search_result()
    assert imin.shape == (B,) and imin.dtype == np.int32 and costs.shape == (B, host.BatchGaitOptimizer.LS_SIZE)
    assert set(ENTRIES) <= set(fake.calls)
    with pytest.raises(AssertionError, match='srbm_gait_closed_loop_advance: argument 1'):
        r.L.srbm_gait_closed_loop_advance(go.g, 1.5, 1, 5, 1, 0)           # (the method converts with int(); the entry itself refuses a float)
    # a gait optimiser of another batch is refused
    other = host.BatchMPC(host.load_config('a1_configuration'), B)
    with pytest.raises(ValueError):
        gait_rollout.GaitRollout(other, go)
    # the module names exactly the three entries, through the library the batch already holds
    text = open(os.path.join(ROOT, 'bilevel-gait-gen_amd', 'gait_rollout.py')).read()
    assert set(re.findall(r'\.(srbm_\w+)\(', text)) == set(ENTRIES)
    go.close(); m.close(); other.close()


def test_gait_fields_from_log_decodes_a_synthetic_record():
    rec = np.arange(64, dtype=np.float64) + 100.0                  # fields 0..57: anything
    rec[58:64] = [1, 1, 0, 0.125, 0, 0]
    assert gait_rollout.gait_fields_from_log(rec) == dict(kind=1, kind_name='gradient', ready=1, lp_status=0, pred_red=0.125, imin=0, winner_cost=0.0)
    rec[58:64] = [1, 0, 2, -3.5, 0, 0]
    d = gait_rollout.gait_fields_from_log(rec)
    assert (d['kind'], d['ready'], d['lp_status'], d['pred_red']) == (1, 0, 2, -3.5)
    rec[58:64] = [2, 0, 0, 0, 7, 41.75]
    assert gait_rollout.gait_fields_from_log(rec) == dict(kind=2, kind_name='line_search', ready=0, lp_status=0, pred_red=0.0, imin=7, winner_cost=41.75)
    rec[58:64] = 0
    d = gait_rollout.gait_fields_from_log(list(rec))
    assert d['kind'] == 0 and d['kind_name'] == 'plain' and not any(d[k] for k in ('ready', 'lp_status', 'pred_red', 'imin', 'winner_cost'))
    assert isinstance(d['imin'], int) and isinstance(d['winner_cost'], float)
    assert sorted(gait_rollout.GAIT_LOG_FIELDS.values()) == list(range(58, 64)) == list(range(host.STEP_LOG_FIELDS['in_contact'].stop, host.STEP_LOG_DOUBLES))
    with pytest.raises(ValueError):
        gait_rollout.gait_fields_from_log(np.zeros((2, 64)))
