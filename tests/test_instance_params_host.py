"""CPU-side checks of the per-instance constructor data (srbm_batch_create_each, BatchMPC.from_configs): the batch-wide fields are checked
before any device is probed, so a mismatch is refused on a machine without a GPU with an error that names the field."""
import ctypes as C
import subprocess
import sys

import pytest

from srbm_loader import host, ROOT


def _arrays(cfgs):
    im = [host._info_model(c) for c in cfgs]
    return (host.MPCInfo * len(cfgs))(*[i for i, _ in im]), (host.Model * len(cfgs))(*[m for _, m in im])


def _cfgs(n=3):
    base = host.load_config('a1_configuration')
    out = []
    for b in range(n):
        c = dict(base)
        c['mass'] = base['mass'] * (1 + 0.05 * b)
        c['friction_coef'] = (0.5, 0.6)[b % 2]
        out.append(c)
    return out


@pytest.fixture(scope='module')
def L():
    host.build()
    return host.lib()


@pytest.mark.parametrize('field,val', [('num_nodes', 21), ('integrator_dt', 0.04), ('swing_height', 0.08), ('foot_offset', 0.02)])
def test_create_each_names_the_mismatched_batch_wide_field(L, field, val):
    cfgs = _cfgs()
    cfgs[2][field] = val
    infos, models = _arrays(cfgs)
    h = C.c_void_p()
    assert L.srbm_batch_create_each(C.byref(h), 3, infos, models, 0) < 0
    msg = L.srbm_last_error().decode()
    assert 'srbm_batch_create_each' in msg and field in msg and 'instance 2' in msg, msg
    assert not h.value


def test_create_each_names_a_mismatched_hip_geometry(L):
    cfgs = _cfgs()
    cfgs[1]['hip_xy'] = [[x + 0.001 for x in row] for row in cfgs[1]['hip_xy']]
    infos, models = _arrays(cfgs)
    h = C.c_void_p()
    assert L.srbm_batch_create_each(C.byref(h), 3, infos, models, 0) < 0
    assert 'hip_xy' in L.srbm_last_error().decode()


def test_create_each_rejects_bad_arguments(L):
    infos, models = _arrays(_cfgs())
    h = C.c_void_p()
    assert L.srbm_batch_create_each(C.byref(h), 0, infos, models, 0) < 0
    assert L.srbm_batch_create_each(C.byref(h), 3, None, models, 0) < 0
    assert 'bad arguments' in L.srbm_last_error().decode()


CHILD = r'''
import ctypes as C, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from srbm_loader import host
import test_instance_params_host as T
L = host.lib()
infos, models = T._arrays(T._cfgs())
h = C.c_void_p()
rc = L.srbm_batch_create_each(C.byref(h), 3, infos, models, 0)
if rc == 0:
    L.srbm_batch_destroy(h)
print('RESULT', rc, L.srbm_last_error().decode() if rc else '')
'''


def test_create_each_with_valid_arguments_gets_to_the_device(L):
    """valid per-instance data pass the checks: without a GPU the call gets as far as the device probe (with one it creates the batch).  In a
    child process, so that this process never opens a device."""
    import os
    p = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'))], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('RESULT')][-1]
    assert line == 'RESULT 0 ' or 'srbm_batch_create_each: no HIP device' in line, line


@pytest.mark.parametrize('field', ['num_nodes', 'integrator_dt', 'swing_height', 'foot_offset', 'hip_xy', 'leg_origins'])
def test_from_configs_rejects_mismatched_batch_wide_configs_before_the_library(monkeypatch, field):
    cfgs = _cfgs()
    cfgs[1][field] = {'num_nodes': 10, 'integrator_dt': 0.02, 'swing_height': 0.1, 'foot_offset': 0.0,
                      'hip_xy': [[0, 0]] * 4, 'leg_origins': [[[0, 0, 0]] * 4] * 4}[field]
    monkeypatch.setattr(host, 'lib', lambda large=False: pytest.fail('the library was called'))
    with pytest.raises(ValueError, match=field):
        host.BatchMPC.from_configs(cfgs)
    with pytest.raises(ValueError):
        host.BatchMPC.from_configs([])
