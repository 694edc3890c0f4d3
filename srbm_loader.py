"""Imports the modules of bilevel-gait-gen_amd/ (the directory name is not a Python identifier): `host` (ctypes binding of the C-ABI) and
`workloads` (seeded instance generators of the BASELINE configurations, sharding), `gait_rollout`, `control_tick`, `mpc_period`, `rollout_summary`, `controller_rollout`, `tick_summary`, `sensors`, `joints`, `wrenches` and `commands` (the entries beside host.py)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'bilevel-gait-gen_amd', file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


host = _load('srbm_host', 'host.py')
workloads = _load('srbm_workloads', 'workloads.py')
workloads.REFERENCE_SOLVER_SETTINGS = host.REFERENCE_SOLVER_SETTINGS       # one definition (host.py), reachable from both
sys.modules[__name__ + '.workloads'] = workloads          # `from srbm_loader.workloads import ...`
sys.modules[__name__ + '.host'] = host
gait_rollout = _load('srbm_gait_rollout', 'gait_rollout.py')
sys.modules[__name__ + '.gait_rollout'] = gait_rollout
control_tick = _load('srbm_control_tick', 'control_tick.py')
sys.modules[__name__ + '.control_tick'] = control_tick
mpc_period = _load('srbm_mpc_period', 'mpc_period.py')
sys.modules[__name__ + '.mpc_period'] = mpc_period
rollout_summary = _load('srbm_rollout_summary', 'rollout_summary.py')
sys.modules[__name__ + '.rollout_summary'] = rollout_summary
controller_rollout = sys.modules[__name__ + '.controller_rollout'] = _load('srbm_controller_rollout', 'controller_rollout.py')
tick_summary = sys.modules[__name__ + '.tick_summary'] = _load('srbm_tick_summary', 'tick_summary.py')
sensors = sys.modules[__name__ + '.sensors'] = _load('srbm_sensors', 'sensors.py')
joints = sys.modules[__name__ + '.joints'] = _load('srbm_joints', 'joints.py')
wrenches = sys.modules[__name__ + '.wrenches'] = _load('srbm_wrenches', 'wrenches.py')
commands = sys.modules[__name__ + '.commands'] = _load('srbm_commands', 'commands.py')
