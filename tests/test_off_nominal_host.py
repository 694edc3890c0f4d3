"""Conditions on the off-nominal cases of tests/off_nominal_kit.py, checked on the references alone (no GPU): that the whole-body QPs are solved and
certified with the rows tight that each family is there for, that enough inverse-kinematics cases converge after large joint steps, and that no
iteration count of a converging foot hangs on a rounding.  They are conditions, not measurements: a seed that breaks one is changed in the kit,
the condition stays.

How the bounds of test_gpu_off_nominal.py follow from what this module prints.  `response` re-evaluates a reference with every input entry moved by a
relative 2^-50 (three seeded draws): what it returns is how far the reference's own result moves when its inputs are rounded differently, the
floor below which "the kernel agrees with the reference" has no meaning.  The kernels do the same few hundred operations per entry in another,
equally plain order (fused multiply-adds, sums in four partial sums, Featherstone's recursion laid out per lane), so their result may differ from
the reference's by some multiple of that floor; the allowance is MARGIN = 1000.

    A, lb, ub, P, w     bound = 1000 x the largest response over the four families, relative to max(1, |.|_inf), capped at the bounds of test_gpu_wbc.py.
                        Printed here: A 3.9e-16, lb 4.1e-15, ub 2.3e-15, w 6.4e-14, P 0 (constants of the configuration: the device must hold the same
                        doubles), so the bounds are A 3.9e-13, lb 4.1e-12, ub 2.3e-12, w 6.4e-11, P 0.  (w moves most where kp 5500 multiplies a joint
                        error of 0.8 rad: 1e5 in units of which 2^-50 is 1e-10 absolute; relative to |w|_inf it is the 6e-14 above.)
    q of the IK         bound = 1000 x the largest response over the cases that converge on all four feet (absolute: q is of order one), capped at 1e-10.
                        Printed here: 2.1e-14, so the bound is 2.1e-11.  A hundred iterations contract every perturbation by 0.9 per iteration, which is
                        why the floor of four hundred iterations stays at a hundred roundings.
    minimiser, torques  1e-6 relative, the bounds of test_gpu_wbc.py: the kernel stops at a residual of 1e-10, not at the minimiser, and the distance
                        between the two is set by the conditioning of the QP, not by rounding.  The interior-point and the polished minimiser of the
                        reference agree to 1e-9 (printed below), three orders inside that bound.
    iteration counts    equal: both deciding error norms of every converging foot are a relative 1e-4 or more away from EPS (asserted below), ten orders
                        above the response."""
import numpy as np

import off_nominal_kit as kit
from oracle_py import qp_solve

ik, wbc = kit.ik, kit.wbc


def test_whole_body_qp_cases_are_solved_certified_and_tight_where_the_family_says():
    cfg = kit.world()[0]
    seen = {tuple(p): 0 for p in kit.PATTERNS}
    for name in kit.QP_FAMILIES:
        fam, ref = kit.qp_family(name), kit.qp_reference(name)
        assert len(ref) == 16
        for b, r in enumerate(ref):
            seen[tuple(fam['contact'][b])] += 1
            assert r['status'] == 0 and r['x'] is not None, (name, b, r['status'], r['info'])
            rel = np.abs(r['x'] - r['x_ipm']).max() / max(1.0, np.abs(r['x']).max())
            assert rel < 1e-8, (name, b, rel)
            if name == 'saturated':
                assert r['torque_tight'] >= 1, (name, b)
            if name == 'friction' and r['nc'] > 0:
                assert r['pyramid_tight'] >= 1, (name, b)
            if name == 'grf' and r['nc'] >= 2:
                assert np.abs(r['fz']).min() < 1e-9, (name, b, r['fz'])
        print('%-9s interior-point iterations %d .. %d, tight inequality rows %d .. %d, interior point against polished %.1e relative'
              % (name, min(r['iters'] for r in ref), max(r['iters'] for r in ref), min(r['tight'] for r in ref), max(r['tight'] for r in ref),
                 max(np.abs(r['x'] - r['x_ipm']).max() / max(1.0, np.abs(r['x']).max()) for r in ref)))
    assert all(n == 4 for n in seen.values()), seen                       # every contact pattern once per family: no case is dropped
    at_bound = sum(int((np.abs(r['fz'] - cfg['force_bound']) < 1e-9).sum()) for r in kit.qp_reference('grf'))
    print('grf: f_z = force_bound on %d feet' % at_bound)
    assert at_bound >= 4
    tumbling = kit.qp_family('tumbling')
    angles = [kit.base_rotation_angle(q[3:7]) for q in tumbling['q']]
    assert max(angles) > np.pi / 2 and tumbling['q'][:, 6].min() < 0, (angles, tumbling['q'][:, 6])
    assert np.all(np.abs(np.linalg.norm(tumbling['q'][:, 3:7], axis=1) - 1) < 1e-15)


def test_the_kit_restates_the_conversion_and_the_torques_of_the_oracle():
    """qp_reference keeps the multipliers the polish starts from, so it restates wbc.solve_qp's conversion to cone form; the torques are taken from the
    polished minimiser, so it restates the formula of wbc.control_action: both held to the oracle bit for bit on one family"""
    cfg, robot, q0, legs = kit.world()
    fam, ref = kit.qp_family('grf'), kit.qp_reference('grf')
    for b in (0, 1, 6, 11, 15):
        r, nc = ref[b], ref[b]['nc']
        x, st = wbc.solve_qp(r['A'], r['lb'], r['ub'], np.diag(r['P']), r['w'], qp_solve)
        assert st == 0 and np.array_equal(x, r['x_ipm']), b
        A, lb, ub, P, w, (M, Cv, g, Js) = kit._build(fam, b)
        ctl, xo, st = wbc.control_action(robot, cfg, fam['q'][b], fam['v'][b], fam['contact'][b], fam['q_des'][b], fam['v_des'][b], fam['fdes'][b, :3 * nc], qp_solve)
        assert np.array_equal(ctl[24:], (M @ xo[:18] - Js.T @ xo[18:] + Cv + g)[6:]), b
        assert np.abs(ctl[24:] - r['tau']).max() < 1e-6, b               # (the torques of the interior-point and of the polished minimiser)


def test_a_negated_base_quaternion_is_the_same_qp_for_the_reference():
    """what the quaternion-sign test of the GPU module relies on: the reference's own data moves by no more than its response"""
    worst = {}
    for a, b in zip(kit.qp_reference('tumbling'), kit.qp_reference('tumbling', negate=True)):
        for k in ('A', 'lb', 'ub', 'P', 'w'):
            fin = np.abs(a[k]) < 1e29
            worst[k] = max(worst.get(k, 0.0), np.abs(a[k][fin] - b[k][fin]).max() / max(1.0, np.abs(a[k][fin]).max()))
        assert np.abs(a['tau'] - b['tau']).max() < 1e-6 * max(1.0, np.abs(a['tau']).max())
    print('tumbling, base quaternion negated: the reference moves by', {k: '%.1e' % v for k, v in worst.items()})
    assert all(worst[k] <= kit.qp_data_bounds()[k] for k in worst), worst


def test_responses_of_the_whole_body_qp_data():
    for name in kit.QP_FAMILIES:
        print('%-9s response of build_qp, relative to max(1, |.|_inf): %s' % (name, {k: '%.1e' % v for k, v in kit.qp_data_response(name).items()}))
    bounds = kit.qp_data_bounds()
    print('bounds of the GPU comparison (1000 x the largest, capped):', {k: '%.1e' % v for k, v in bounds.items()})
    for k, cap in kit.DATA_CAPS.items():
        assert bounds[k] < cap, (k, bounds[k])                            # the cap is not what binds: the bounds are the reference's floor
    assert bounds['P'] == 0.0


def test_inverse_kinematics_cases_converge_after_large_steps_and_no_count_hangs_on_a_rounding():
    legs, c, ref = kit.world()[3], kit.ik_cases(), kit.ik_reference()
    assert len(ref) == 18
    converged, with_large_steps = [], []
    for b, (q, iters, ok) in enumerate(ref):
        qi, iti, feet = kit.ik_instrumented(legs, c['state'][b], c['ee_des'][b], c['q_guess'][b])
        assert np.array_equal(q, qi) and list(iters) == list(iti), b                      # the instrumented copy is the loop of the oracle
        for e, (last, prev, big) in enumerate(feet):
            if iters[e] < ik.IT_MAX:
                assert last < ik.EPS * (1 - 1e-4) and (prev is None or prev > ik.EPS * (1 + 1e-4)), (b, e, last, prev)
        if max(iters) < ik.IT_MAX:
            converged.append(b)
            if sum(f[2] for f in feet) > 0:
                with_large_steps.append(b)
        print('ik case %2d: iterations %s, iterations with a joint step above %.3f rad %s' % (b, list(iters), kit.SMALL_STEP, [f[2] for f in feet]))
    assert converged == kit.ik_converged_cases()
    assert len(converged) >= 12 and len(with_large_steps) >= 4, (converged, with_large_steps)
    resp = kit.ik_response()
    for b in converged:
        print('ik case %2d: response of q %.1e' % (b, resp[b][0]))
        assert not resp[b][1], b                                                          # the counts do not move under the perturbation
    print('largest response of q over the %d cases that converge on all feet: %.1e; bound of the GPU comparison %.1e'
          % (len(converged), max(r for r, m in resp.values()), kit.ik_bound()))
    assert kit.ik_bound() < kit.IK_CAP
