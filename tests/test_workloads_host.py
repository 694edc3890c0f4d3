"""The two package helpers every GPU test and developer script starts from, on the CPU: workloads.instances against the written-out seeding idiom
(bytes), BatchMPC.cold_start against the written-out call sequence (a recording subclass: no library, no GPU)."""
import numpy as np
import pytest

from oracle_py import load_config
from srbm_loader import host, workloads
from srbm_loader.workloads import config_b_instance, config_c_instance, config_d_instance, heterogeneous_configs, instances

CASES = [(config_b_instance, 'a1_configuration'), (config_c_instance, 'a1_gait_opt_config'), (config_d_instance, 'a1_config_distr_rejection')]


def idiom(cfgs, make_inst, ids):
    states, ees = zip(*[make_inst(c, b) for c, b in zip(cfgs, ids)])
    return np.array(states), np.array(ees).reshape(len(ids), 12)


def assert_batch(got, want, B):
    for g, w, width in zip(got, want, (13, 12)):
        assert g.shape == (B, width) and g.dtype == np.float64 and g.flags['C_CONTIGUOUS']
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize('make_inst,cfgname', CASES, ids=['B', 'C', 'D'])
@pytest.mark.parametrize('ids', [5, range(2, 7), [b % 3 for b in range(7)]], ids=['int', 'range', 'modulo'])
def test_instances_is_the_seeding_idiom_byte_for_byte(make_inst, cfgname, ids):
    cfg = load_config(cfgname)
    want_ids = list(range(ids)) if isinstance(ids, int) else list(ids)
    assert_batch(instances(cfg, make_inst, ids), idiom([cfg] * len(want_ids), make_inst, want_ids), len(want_ids))


def test_instances_with_one_config_per_instance():
    base = load_config()
    cfgs = heterogeneous_configs(base, [base['Q_srbd_diag'], load_config('a1_config_distr_rejection')['Q_srbd_diag']], 5)
    assert_batch(instances(cfgs, config_b_instance, 5), idiom(cfgs, config_b_instance, range(5)), 5)
    assert_batch(instances(cfgs, config_b_instance, [4, 3, 2, 1, 0]), idiom(cfgs, config_b_instance, [4, 3, 2, 1, 0]), 5)
    with pytest.raises(ValueError):
        instances(cfgs, config_b_instance, 4)


def test_config_d_feet_are_the_nominal_feet_and_not_shared():
    cfg = load_config('a1_config_distr_rejection')
    _, ee = config_d_instance(cfg, 0)
    assert ee.flags.writeable and not workloads.EE_NOMINAL.flags.writeable and np.array_equal(ee, [[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]])
    assert workloads.REFERENCE_SOLVER_SETTINGS == host.REFERENCE_SOLVER_SETTINGS == (1e-15, 1e-15, 1e-10, 200)


class Recorder(host.BatchMPC):
    """BatchMPC without a library: the constructors and the four methods of the cold start only record their calls"""

    def __init__(self, cfg, batch, device=0, large=None):
        self.calls = [('__init__', cfg, batch, device, large)]

    @classmethod
    def from_configs(cls, cfgs, device=0, large=None):
        g = cls(None, len(cfgs))
        g.calls = [('from_configs', cfgs, device, large)]
        return g

    def set_state_trajectory_warm_start(self, states):
        self.calls.append(('set_state_trajectory_warm_start', states))

    def set_solver_tolerances(self, *a):
        self.calls.append(('set_solver_tolerances',) + a)

    def set_solver_step_rule(self, *a):
        self.calls.append(('set_solver_step_rule',) + a)

    def create_initial_run(self, states, ees):
        self.calls.append(('create_initial_run', states, ees))

    def close(self):
        pass


CFG = {'num_nodes': 20}
STATES, EES = np.arange(39.0).reshape(3, 13), np.arange(36.0).reshape(3, 12)


def test_cold_start_call_sequence():
    g = Recorder.cold_start(CFG, STATES, EES, mode=(1e-5, 0.1))
    assert isinstance(g, Recorder)
    assert g.calls == [('__init__', CFG, 3, 0, None), ('set_state_trajectory_warm_start', STATES), ('set_solver_tolerances', 1e-15, 1e-15, 1e-10, 200),
                       ('set_solver_step_rule', 1e-5, 0.1), ('create_initial_run', STATES, EES)]
    assert g.calls[1][1] is STATES and g.calls[4][1] is STATES and g.calls[4][2] is EES        # handed on as given


def test_cold_start_without_a_mode_leaves_the_step_rule_alone():
    g = Recorder.cold_start(CFG, STATES, EES)
    assert [c[0] for c in g.calls] == ['__init__', 'set_state_trajectory_warm_start', 'set_solver_tolerances', 'create_initial_run']


def test_cold_start_without_the_initial_run():
    g = Recorder.cold_start(CFG, STATES, None, mode=(0.0, 0.0), initial_run=False)
    assert [c[0] for c in g.calls] == ['__init__', 'set_state_trajectory_warm_start', 'set_solver_tolerances', 'set_solver_step_rule']
    assert g.calls[-1] == ('set_solver_step_rule', 0.0, 0.0)


def test_cold_start_of_one_state_or_a_list_of_states_sizes_the_batch():
    s0 = np.arange(13.0)
    assert Recorder.cold_start(CFG, s0, EES[0]).calls[0] == ('__init__', CFG, 1, 0, None)
    assert Recorder.cold_start(CFG, [s0] * 4, EES[0]).calls[0] == ('__init__', CFG, 4, 0, None)


def test_cold_start_of_a_list_of_configs_goes_through_from_configs():
    cfgs = [dict(CFG, mass=m) for m in (10.0, 11.0, 12.0)]
    g = Recorder.cold_start(cfgs, STATES, EES, mode=(0.0, 0.1))
    assert g.calls[0] == ('from_configs', cfgs, 0, None)
    assert [c[0] for c in g.calls[1:]] == ['set_state_trajectory_warm_start', 'set_solver_tolerances', 'set_solver_step_rule', 'create_initial_run']


def test_cold_start_passes_large_and_device_on():
    assert Recorder.cold_start(CFG, STATES, EES, large=True, device=3).calls[0] == ('__init__', CFG, 3, 3, True)
    cfgs = [CFG] * 3
    assert Recorder.cold_start(cfgs, STATES, EES, large=False, device=2).calls[0] == ('from_configs', cfgs, 2, False)
