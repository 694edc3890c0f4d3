"""The MPC period of the closed-loop protocols without a GPU (include/srbm_rti.h: srbm_plant_set_period; bilevel-gait-gen_amd/mpc_period.py):

    a  RestatementLoop (tests/closed_loop_kit.py) given p = dt is RestatementLoop given no period, bit for bit;
    b  the inputs of tests/test_gpu_mpc_period.py stay within their conditions on the restatement alone: every run Solved, more than one (n, m) per
       configuration, gradient ready and LP solved at runs 4 and 9, the two cheapest candidates of each line search more than 1e-4 apart;
    c  the two entries in the header and in the prototype table, and the wrapper's shape refusals before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from closed_loop_kit import GAIT_CASES, GAIT_FREQ, GAIT_RUNS, GRADIENT, LINE_SEARCH, NO_GAIT, PUSH, SUB, RestatementLoop, plain_case
from oracle_py import load_config
from srbm_loader import ROOT, host, mpc_period
from srbm_loader.workloads import EE_NOMINAL
from test_abi_prototypes import HANDLE, StandIn

ENTRIES = ('srbm_plant_set_period', 'srbm_plant_get_period')


def test_period_loop_at_the_node_step_is_the_restatement_loop_bitwise():
    cfg = load_config('a1_configuration')
    s0 = np.array(cfg['srb_init'], float)
    args = (cfg, s0, EE_NOMINAL, GAIT_FREQ, SUB, 1, 0.12, PUSH)
    a, b = RestatementLoop(*args), RestatementLoop(*args, period=cfg['integrator_dt'])
    kinds = []
    for r in range(1, GAIT_RUNS + 1):
        oa, ob = a.run(), b.run()
        assert set(oa) == set(ob)
        for k in oa:
            va, vb = oa[k], ob[k]
            assert (va is None) == (vb is None), (r, k)
            if va is not None:
                assert np.asarray(va).tobytes() == np.asarray(vb).tobytes(), (r, k)
        assert a.o.states().tobytes() == b.o.states().tobytes() and a.x.tobytes() == b.x.tobytes(), r
        assert a.o.x().tobytes() == b.o.x().tobytes(), r
        kinds.append(oa['kind'])
    assert kinds == [0, 0, 0, 1, 2, 0, 0, 0, 1, 2, 0]                      # (both line searches searched: the comparison covered all three kinds)


@pytest.mark.parametrize('name', ['config_b', 'config_d'])
def test_plain_loop_inputs_stay_solved_and_change_size(name):
    cfg, states, ees, periods, push_times, impulses, runs, adv = plain_case(name)
    assert np.all(periods > 0) and np.all(periods < cfg['num_nodes'] * cfg['integrator_dt'])
    for advance_time in adv:
        sizes = set()
        for b in range(len(periods)):
            loop = RestatementLoop(cfg, states[b], ees[b], NO_GAIT, SUB, advance_time, push_times[b], impulses[b], periods[b])
            for r in range(1, runs + 1):
                out = loop.run()
                assert out['kind'] == 0 and loop.o.stats()['status'] == 0, (name, advance_time, b, r, loop.o.stats()['status'])
                sz = loop.o.sizes()
                sizes.add((sz['n'], sz['m']))
        print(name, advance_time, sorted(sizes))
        assert len(sizes) > 1, sizes


@pytest.mark.parametrize('cfgname,push_time,period', GAIT_CASES)
def test_gait_loop_inputs_have_ready_gradients_and_clear_line_searches(cfgname, push_time, period):
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    loop = RestatementLoop(cfg, s0, EE_NOMINAL, GAIT_FREQ, SUB, 1, push_time, PUSH, period)
    gaps = []
    for r in range(1, GAIT_RUNS + 1):
        out = loop.run()
        if r in (4, 9):
            assert out['kind'] == GRADIENT and out['ready'] and out['step'] is not None, (r, out['kind'], out['ready'])
        if r in (5, 10):
            assert out['kind'] == LINE_SEARCH, (r, out['kind'])
            srt = np.sort(out['costs'])
            gaps.append((srt[1] - srt[0]) / max(1.0, abs(srt[0])))
    print(cfgname, period, 'gaps of the two cheapest candidates', gaps)
    assert len(gaps) == 2 and min(gaps) > 1e-4, gaps


def test_the_entries_are_in_the_header_and_in_the_prototype_table():
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read(), flags=re.S)
    assert re.search(r'^int srbm_plant_set_period\(srbm_batch\* h, const double\* period\);', text, flags=re.M)
    assert re.search(r'^int srbm_plant_get_period\(srbm_batch\* h, double\* period\);', text, flags=re.M)
    for name in ENTRIES:
        assert host.PROTOTYPES[name] == (C.c_int, (C.c_void_p, C.POINTER(C.c_double))), name
    # the header says that the open-loop entries ignore the setting
    raw = open(os.path.join(ROOT, 'include', 'srbm_rti.h')).read()
    assert re.search(r'open-loop entries[^.]*ignore srbm_plant_set_period', raw)


def test_wrapper_broadcasts_and_refuses_wrong_shapes_before_the_library(monkeypatch):
    fake = StandIn(host.PROTOTYPES, dict(N=50, nu=160, samples=120, knots=32))
    monkeypatch.setitem(host._libs, host.LIB_PATH, fake)
    B = 3
    m = host.BatchMPC(host.load_config('a1_configuration'), B)
    m.h = C.c_void_p(HANDLE)
    assert np.array_equal(mpc_period.period_array(0.013, B), np.full(B, 0.013)) and np.array_equal(mpc_period.period_array([0.02], B), np.full(B, 0.02))
    per = np.array([0.05, 0.025, 0.013])
    assert np.array_equal(mpc_period.period_array(per, B), per) and mpc_period.period_array([1, 2, 3], B).dtype == np.float64
    for ok in (None, 0.013, np.float32(0.02), 1, per, list(per), per[::-1]):          # (a reversed view: made contiguous)
        mpc_period.plant_set_period(m, ok)
    mpc_period.plant_set_period(m)
    assert fake.calls.count('srbm_plant_set_period') == 8
    for bad in (np.zeros(B + 1), np.zeros(B - 1), np.zeros((B, 1)), np.zeros((1, B)), [], np.zeros((B, B))):
        with pytest.raises(ValueError, match='period'):
            mpc_period.plant_set_period(m, bad)
    assert fake.calls.count('srbm_plant_set_period') == 8                    # refused before the library was called
    out = mpc_period.plant_period(m)
    assert out.shape == (B,) and out.dtype == np.float64 and 'srbm_plant_get_period' in fake.calls
    # the module names exactly the two entries, through the library the batch already holds
    text = open(os.path.join(ROOT, 'bilevel-gait-gen_amd', 'mpc_period.py')).read()
    assert set(re.findall(r'\.(srbm_\w+)\(', text)) == set(ENTRIES)
    m.close()
