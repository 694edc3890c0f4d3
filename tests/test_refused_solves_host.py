"""CPU side of tests/test_gpu_refused_solves.py: what the schedules of tests/refused_solves_kit.py ask of kernel 1, by the oracle's sizes, and the
search that gives the not-ready comparison its teeth.  (The refusals of srbm_export_qp / srbm_gait_get_param_partials / srbm_gait_line_search
read the instance record or the handle on a device: every one of them is in the GPU file.)"""
import numpy as np
import pytest

import refused_solves_kit as kit


@pytest.fixture(scope='module')
def reached():
    return kit.reach_oracle()


def test_the_state_has_five_contact_times_per_foot_and_fits(reached):
    cfg, o, t = reached
    counts = [len(o.contact_times(e)[0]) for e in range(4)]
    assert counts == [5, 5, 5, 5]
    own = [o.contact_times(e)[0] for e in range(4)]
    nu, samples, knots = kit.oracle_sizes(o, t + cfg['integrator_dt'], own)
    assert kit.exits(nu, samples, knots) == set(), (nu, samples, knots)


def test_which_capacity_exit_each_schedule_reaches(reached):
    cfg, o, t = reached
    tn = t + cfg['integrator_dt']
    counts = [5] * 4
    nu, samples, knots = kit.oracle_sizes(o, tn, kit.uniform_times(counts, kit.PHASE_VARIABLES))
    assert (nu, samples, knots) == (176, 120, 16) and kit.exits(nu, samples, knots) == {'nu'}            # spline variables, alone
    nu, samples, knots = kit.oracle_sizes(o, tn, kit.uniform_times(counts, kit.PHASE_BOTH))
    assert (nu, samples, knots) == (204, 140, 19) and kit.exits(nu, samples, knots) == {'nu', 'samples'}


def test_no_schedule_of_the_grid_reaches_the_sample_or_the_knot_exit_alone(reached):
    cfg, o, t = reached
    tn = t + cfg['integrator_dt']
    seen = [kit.oracle_sizes(o, tn, kit.uniform_times([5] * 4, p)) for p in kit.GRID]
    for p, (nu, samples, knots) in zip(kit.GRID, seen):
        ex = kit.exits(nu, samples, knots)
        assert 'knots' not in ex and ex != {'samples'}, (p, nu, samples, knots)
        # 10 samples and 12 force variables per sampled stance phase: the samples never overflow before the variables
        assert nu >= 12 * (samples // 10), (p, nu, samples)
    assert max(k for _, _, k in seen) == 19
    # one foot squeezed, the others on their own times: its table grows, the sizes stay inside every capacity
    own = [o.contact_times(e)[0] for e in range(4)]
    for f in range(4):
        times = [own[e] if e != f else 0.001 * np.arange(5) for e in range(4)]
        nu, samples, knots = kit.oracle_sizes(o, tn, times)
        assert kit.exits(nu, samples, knots) == set() and knots == 16, (f, nu, samples, knots)


def test_reapplying_the_contact_times_moves_interior_knots_of_this_state(reached):
    """The teeth of the not-ready comparisons: on the tables of the state the GPU cases start from, srbm_apply_contact_times with the table's own
    contact times returns other bits for at least one stance-interior knot of every foot (0.3 + 0.1 + 0.1 against 0.3 + 0.3 / 3 + 0.3 / 3 and the
    like), and never for a contact knot.  A line search that rewrote a not-ready instance's schedule therefore cannot equal the plain update."""
    cfg, o, t = reached
    for e in range(4):
        kn = o.knots(e)
        kinds = kit.knot_kinds(kn)
        again = kit.reapply_contact_times(kn['times'], kinds)
        moved = np.nonzero(again != kn['times'])[0]
        assert len(moved) >= 1 and np.all(kinds[moved] >= 2), (e, moved, kinds)
        assert np.abs(again - kn['times']).max() <= 4 * np.spacing(kn['times'].max())       # a rounding, not another schedule
        assert np.array_equal(kit.reapply_contact_times(again, kinds), again)                 # and the formula is idempotent
