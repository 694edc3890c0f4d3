"""The whole-body QP kernel (srbm_k_qp_control: wbc_build_qp and wbc_solve_qp, csrc/srbm_wbc.hiph) and the inverse kinematics (ik_solve_foot,
csrc/srbm_ik.hiph) against their references OFF NOMINAL: the cases of tests/off_nominal_kit.py -- torque, friction and force rows tight, feet at zero
force, every contact pattern, bases rolled past 90 degrees, joint rates of 6 rad/s, IK solves that begin with joint steps above 0.125 rad.
tests/test_off_nominal_host.py checks the conditions on those cases and says where every bound below comes from: the QP data and the joint angles
are held to 1000 x the reference's own response to a rounding of its inputs, the minimiser and the torques to the 1e-6 of test_gpu_wbc.py, the
iteration counts of the IK to equality.  No case is skipped, filtered by the device's status or retried.

Observed on the device (MI355X), printed by the tests next to the bounds: see DESIGN.md section 4."""
import functools

import numpy as np
import pytest

import off_nominal_kit as kit
from control_tick_kit import assert_tick_equals_chain, chain_qp, chain_targets, reconstruct_state
from srbm_loader import host
from srbm_loader.control_tick import ControlTick
from srbm_loader.workloads import config_b_instance, instances

pytestmark = pytest.mark.gpu
ik = kit.ik
DATA = ('A', 'lb', 'ub', 'P', 'w')


@functools.lru_cache(None)
def device_qp(name, large=False, negate=False):
    """one launch of 16 waves: (control, qp_sol, status, iterations, dump) of the family on the device"""
    cfg = kit.world()[0]
    fam = kit.negated_base_quaternion(kit.qp_family(name)) if negate else kit.qp_family(name)
    g = host.BatchMPC(cfg, 16, large=large)
    out = g.qp_control(fam['q'], fam['v'], fam['contact'], fam['q_des'], fam['v_des'], fam['fdes'], dump=True)
    g.close()
    return fam, out


def data_errors(qp, ref):
    """per quantity the largest error over the 16 cases, relative to max(1, |reference|_inf); the entries past (m, n) are zero and the open lower
    bounds are open"""
    worst = dict.fromkeys(DATA, 0.0)
    for b, r in enumerate(ref):
        n, m = r['n'], r['m']
        assert np.all(qp['A'][b, m:, :] == 0) and np.all(qp['A'][b, :, n:] == 0) and np.all(qp['P'][b, n:] == 0) and np.all(qp['w'][b, n:] == 0), b
        fin = np.abs(r['lb']) < 1e29
        assert np.all(qp['lb'][b, :m][~fin] < -1e29) and np.all(np.abs(qp['lb'][b, :m][fin]) < 1e29), b
        for k, dev, want in (('A', qp['A'][b, :m, :n], r['A']), ('lb', qp['lb'][b, :m][fin], r['lb'][fin]), ('ub', qp['ub'][b, :m], r['ub']),
                             ('P', qp['P'][b, :n], r['P']), ('w', qp['w'][b, :n], r['w'])):
            worst[k] = max(worst[k], np.abs(dev - want).max() / max(1.0, np.abs(want).max()))
    return worst


def check_data(where, qp, ref):
    worst, bounds = data_errors(qp, ref), kit.qp_data_bounds()
    print('%s: QP data against build_qp, relative to max(1, |.|_inf): %s' % (where, ', '.join('%s %.1e (bound %.1e)' % (k, worst[k], bounds[k]) for k in DATA)))
    for k in DATA:
        assert worst[k] <= bounds[k], (where, k, worst[k], bounds[k])


def check_solve(where, fam, out, ref):
    ctl, sol, st, iters, qp = out
    tb = np.array(kit.world()[0]['torque_bounds'], float)
    ex = et = 0.0
    print('%s: interior-point iterations min %d median %d max %d, solves with status 1: %d, other statuses: %s'
          % (where, iters.min(), np.median(iters), iters.max(), int((st == 1).sum()), [(b, int(s)) for b, s in enumerate(st) if s > 1]))
    for b, r in enumerate(ref):
        n = r['n']
        assert st[b] <= 1, (where, b, int(st[b]), int(iters[b]))                     # the reference solves every case: 2 or 8 is the kernel's failure
        ex = max(ex, np.abs(sol[b, :n] - r['x']).max() / max(1.0, np.abs(r['x']).max()))
        et = max(et, np.abs(ctl[b, 24:] - r['tau']).max() / max(1.0, np.abs(r['tau']).max()))
        assert np.all(sol[b, n:] == 0), (where, b)
        assert np.all(np.abs(ctl[b, 24:]) <= tb + 1e-6), (where, b, ctl[b, 24:])
    print('%s: minimiser against the certified minimiser %.1e relative, torques %.1e relative (bounds 1e-6)' % (where, ex, et))
    assert ex < 1e-6 and et < 1e-6, (where, ex, et)
    assert ctl[:, :12].tobytes() == fam['q_des'][:, 7:].tobytes() and ctl[:, 12:24].tobytes() == fam['v_des'][:, 6:].tobytes(), where


@pytest.mark.parametrize('name', kit.QP_FAMILIES)
def test_assembled_qp_matches_build_qp(name):
    fam, out = device_qp(name)
    check_data(name, out[4], kit.qp_reference(name))


@pytest.mark.parametrize('name', kit.QP_FAMILIES)
def test_solution_matches_the_certified_minimiser(name):
    fam, out = device_qp(name)
    check_solve(name, fam, out, kit.qp_reference(name))


def test_tumbling_on_the_large_build():
    fam, out = device_qp('tumbling', large=True)
    check_data('tumbling, large build', out[4], kit.qp_reference('tumbling'))
    check_solve('tumbling, large build', fam, out, kit.qp_reference('tumbling'))


def test_the_base_quaternions_sign_does_not_matter():
    """q and -q are one attitude: the linear cost (the only place the attitude error log3 enters) and the torques do not depend on the representative"""
    (fam, out), (nfam, nout) = device_qp('tumbling'), device_qp('tumbling', negate=True)
    assert np.all(nfam['q'][:, 3:7] == -fam['q'][:, 3:7])
    bound, dw, dt = kit.qp_data_bounds()['w'], 0.0, 0.0
    for b, r in enumerate(kit.qp_reference('tumbling')):
        n = r['n']
        assert out[2][b] <= 1 and nout[2][b] <= 1, (b, int(out[2][b]), int(nout[2][b]))
        dw = max(dw, np.abs(out[4]['w'][b, :n] - nout[4]['w'][b, :n]).max() / max(1.0, np.abs(r['w']).max()))
        dt = max(dt, np.abs(out[0][b, 24:] - nout[0][b, 24:]).max() / max(1.0, np.abs(r['tau']).max()))
    print('tumbling, base quaternion negated: w moves by %.1e relative (bound %.1e), the torques by %.1e (bound 1e-6)' % (dw, bound, dt))
    assert dw <= bound and dt < 1e-6
    check_data('tumbling, base quaternion negated', nout[4], kit.qp_reference('tumbling', negate=True))
    check_solve('tumbling, base quaternion negated', nfam, nout, kit.qp_reference('tumbling', negate=True))


def test_inverse_kinematics_after_large_joint_steps():
    cfg, robot, q0, legs = kit.world()
    c, ref = kit.ik_cases(), kit.ik_reference()
    B = len(ref)
    g = host.BatchMPC(cfg, B)
    qs, iters, st = g.inverse_kinematics(c['state'], c['ee_des'].reshape(B, 12), c['q_guess'])
    fk = g.forward_kinematics(qs)
    converged = kit.ik_converged_cases()
    bound, eq, ef = kit.ik_bound(), 0.0, 0.0
    for b, (qo, ito, ok) in enumerate(ref):
        first_bad = ito.index(ik.IT_MAX) if ik.IT_MAX in ito else 3
        assert ok == (st[b] == 0) and list(iters[b][:first_bad + 1]) == ito[:first_bad + 1], (b, list(iters[b]), ito)
        for e in range(first_bad + 1, 4):         # after a foot at IT_MAX the base pose is chaotic in the last bits: convergence only (test_gpu_ik.py)
            assert (iters[b][e] < ik.IT_MAX) == (ito[e] < ik.IT_MAX), (b, list(iters[b]), ito)
        if b in converged:
            eq, ef = max(eq, np.abs(qs[b] - qo).max()), max(ef, np.abs(fk[b] - c['ee_des'][b]).max())
    print('inverse kinematics, %d of %d cases converge on all feet: |q - q_ref|_inf %.1e (bound %.1e), FK(q) against the targets %.1e (bound 2e-5)'
          % (len(converged), B, eq, bound, ef))
    assert eq <= bound and ef < 2e-5


def test_a_tick_on_a_tumbling_measurement_equals_the_chain():
    """one tick of a cold-started batch whose measured (q, v) are the tumbling family's: the one-call tick and the chain of the single entries run the
    same code on it, bit for bit; what the tick hands to the MPC (position and linear momentum) is ReconstructState of that measurement"""
    B = 16
    cfg = host.load_config('a1_configuration')
    fam = kit.qp_family('tumbling')
    states, ees = instances(cfg, config_b_instance, B)
    base = host.BatchMPC.cold_start(cfg, states, ees)
    q0 = np.tile(np.array(cfg['init_config'], float), (B, 1))
    t = base.get_trajectory(0, 1)[0].init_time + 0.2985 + 4e-4 * (np.arange(B) % 2)
    ref = chain_qp(base, chain_targets(base, t, q0), fam['q'], fam['v'])
    g = base.clone()
    T = ControlTick(g)
    T.reset(q0)
    out = T.tick(fam['q'], fam['v'], t)
    print('tick on the tumbling measurement: target statuses %s, QP statuses %s, iterations %s'
          % (out['targets_status'].tolist(), out['qp_status'].tolist(), out['qp_iters'].tolist()))
    assert_tick_equals_chain(out, ref, 'tick on the tumbling measurement')
    s = reconstruct_state(fam['q'], fam['v'], cfg['mass'], np.array(cfg['Ir'], float))
    assert out['state'][:, :6].tobytes() == s[:, :6].tobytes()
