"""The oracle with a final cost that is not the tracking cost (no GPU): orc_mpc_set_costs / OracleMPC.set_costs and the cost sets of
tests/cost_variants_kit.py, before the device is held to them (tests/test_gpu_cost_variants.py).  N = 20, one Config-B instance per set."""
import numpy as np
import pytest

from cost_variants_kit import SETS, cost_set, expected_cost_blocks, plain_costs, tracking_as_final
from oracle_py import OracleMPC, load_config
from srbm_loader.workloads import config_b_instance

CFG = load_config('a1_configuration')
assert CFG['num_nodes'] == 20


def started(inst, costs=None):
    """an oracle after its cold start on Config-B instance `inst`, the costs installed before it"""
    state, ee = config_b_instance(CFG, inst)
    o = OracleMPC(CFG)
    if costs is not None:
        o.set_costs(*costs)
    o.set_warmstart(state)
    assert o.initial_run(state, ee) <= 1
    return o


def step(o, i):
    """one open-loop RTI step on the oracle's own path (test/gait_opt_playground.cpp:113-126)"""
    t = i * CFG['integrator_dt']
    state = o.states()[1]
    ee = np.array([[o.ee_value(e, 1, c, t) for c in range(3)] for e in range(4)])
    return o.rti(state, t, ee)


def outputs(o):
    s = o.stats()
    return dict(x=o.x(), qp_x=o.qp_x(), z=o.z(), s=o.s(), states=o.states(), stats=np.array([s[k] for k in sorted(s) if k != 'box'] + list(s['box'])))


def assert_same_bytes(a, b, where):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (where, k)


def test_set_costs_with_the_constructors_costs_changes_no_bit():
    """the new entry is the three setters and nothing else: given what orc_mpc_create sets, every output keeps its bytes"""
    a, b = started(0), started(0, plain_costs(CFG))
    assert_same_bytes(outputs(a), outputs(b), 'cold start')
    for i in range(2):
        assert step(a, i) == step(b, i)
        assert_same_bytes(outputs(a), outputs(b), 'step %d' % i)


@pytest.mark.parametrize('name', SETS)
def test_assembled_cost_is_the_block_diagonal_of_the_set(name):
    """P and q of the exported QP: Q + 1e-3 I and w on nodes 0 .. N-1, Phi + 1e-3 I and Phi_w on node N, nothing between the nodes or between states
    and spline variables.  A clone keeps the costs."""
    costs = cost_set(CFG, name)
    o = started(SETS.index(name), costs)
    assert step(o, 0) <= 1
    c = o.clone()
    nx = 12 * (CFG['num_nodes'] + 1)
    Pe, qe = expected_cost_blocks(CFG, costs)
    for which, h in (('original', o), ('clone', c)):
        if h is c:
            assert step(o, 1) == step(c, 1)
            assert_same_bytes(outputs(o), outputs(c), 'clone, set %s' % name)
        _, _, P, q = h.qp_dense()
        assert np.abs(P[:nx, :nx] - Pe).max() <= 1e-15, (name, which, np.abs(P[:nx, :nx] - Pe).max())
        assert np.abs(q[:nx] - qe).max() <= 1e-15, (name, which, np.abs(q[:nx] - qe).max())
        assert not P[:nx, nx:].any() and not P[nx:, :nx].any() and not q[nx:].any(), (name, which)
    # the set is what its table says: the last node's block is not the tracking block
    assert np.abs(Pe[-12:, -12:] - Pe[:12, :12]).max() > 1.0 and np.abs(qe[-12:] - qe[:12]).max() > 1.0, name


@pytest.mark.parametrize('name', SETS)
def test_final_cost_moves_the_minimiser(name):
    """a kernel that took Q, w on the last node would be seen: from one linearisation point (cold start and 2 steps under the set), the QP of the
    set and the QP with Phi, Phi_w := Q, w have raw minimisers more than 1e-2 apart (of the largest entry)"""
    costs = cost_set(CFG, name)
    o = started(SETS.index(name), costs)
    for i in range(2):
        assert step(o, i) <= 1
    c = o.clone()
    c.set_costs(*tracking_as_final(costs))
    assert step(o, 2) <= 1 and step(c, 2) <= 1
    A, b, _, _ = o.qp_dense()
    Ac, bc, _, _ = c.qp_dense()
    assert np.array_equal(A, Ac) and np.array_equal(b, bc)            # the same constraints: only the cost differs
    xa, xb = o.qp_x(), c.qp_x()
    d = np.abs(xa - xb).max() / np.abs(xa).max()
    print('set %s: the raw minimiser moves by %.3g of its largest entry when the final cost becomes the tracking cost' % (name, d))
    assert d > 1e-2, (name, d)
