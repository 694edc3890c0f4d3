"""The contact-time LP kernel (srbm_k_gait_lp, csrc/srbm_gait_lp.hiph) against an exact LP solver (tests/lp_reference.py) OFF the nominal
schedules: feet with up to 16 contact times and different counts, the capacity exits, every position of the next contact time, gaps below
the minimum phase, infeasible LPs, and gradients of any size.  The schedules reach the device as trajectory records
(srbm_set_warm_start_trajectory), the gradients through srbm_gait_set_gradient; every case is an instance of one of two 128-instance batches
on ONE N = 20 cold start, solved once and shared by the tests below (nothing here changes them).

Bounds: lp_reference.value_bound (E, from the kernel's stop test by weak duality), rows <= 1e-9 (the kernel stops at 1e-10; rows of size ~5
evaluated in numpy), slack of a row with marginal >= tau = 1e-3 C at most 2 E / tau, entries at a nondegenerate vertex 16 * 2 E / tau (a chain
of at most 16 links).

Observed on an MI355X (worst over the cases, value error / E and entry error / bound): 3.1e-2 and 2.9e-5 over the drawn cases, 1.6e-2 and 3.1e-5
over the scale cases.  Before the kernel iterated on c / max(1, |c|_inf) the scale cases ended with lp_status 2 at |c|_inf = 1e8, 1e10 and 1e12 (all
three directions; solved at 1e-2 ... 1e6), and so did one drawn case with entries of ~1e8."""
import functools

import numpy as np
import pytest

import lp_reference as R
from gpu_kit import same_bytes
from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import EE_NOMINAL

pytestmark = pytest.mark.gpu

SEED = 20
B = 128
NV = host.BatchGaitOptimizer.NV
ERR_CAPACITY = 16                      # SRBM_ERR_CAPACITY (csrc/srbm_types.h)
SCALES = (-2, 0, 2, 4, 6, 8, 10, 12)


def infeasible_case(rng, counts, interleave):
    """a gap below the minimum phase between two PINNED contact times: the next contact time of the longest foot is a touch-down at index 2, so
    0 (start) and 1 (before the touch-down) are frozen, and the row between them asks for 0 <= gap - 0.2 < 0"""
    cts, kinds = R.draw_schedule(rng, counts)
    ee = int(np.argmax(counts))
    cts[ee][1:] += 0.15 - (cts[ee][1] - cts[ee][0])
    if kinds[ee][2] != R.TD:
        kinds[ee] = 1 - kinds[ee]
    tnow = rng.uniform(cts[ee][1], cts[ee][2])
    c = R.draw_gradient(rng, int(np.sum(counts)), 'generic')
    return R.make_case(counts, cts, kinds, tnow, c, [R.knot_table(rng, cts[e], kinds[e], interleave) for e in range(4)], 'infeasible', 'generic')


def overflow_case(rng, counts):
    """more contact times than a foot's 16 lanes or an instance's 32 entries hold: no LP, no reference"""
    cts, kinds = R.draw_schedule(rng, counts)
    nv = int(np.sum(counts))
    return dict(counts=tuple(counts), cts=cts, kinds=kinds, tnow=0.1, c=rng.normal(size=nv)[:NV], nv=nv, overflow=True,
                table=[R.knot_table(rng, cts[e], kinds[e], False) for e in range(4)])


def scaled(case, k):
    """the same LP with the cost normalised to |c|_inf = 1 and multiplied by 10**k: the minimiser stays, value and marginals scale"""
    s = 10.0 ** k / np.abs(case['c']).max()
    out = dict(case, c=case['c'] * s, scale_k=k)
    out['ref'] = dict(case['ref'], f=case['ref']['f'] * s, y=case['ref']['y'] * s, z=case['ref']['z'] * s)
    return R.bounds_of(out)


@functools.lru_cache(None)
def cases():
    """(batch A, batch B, index tables): all cases and their references, drawn on the host from one seeded generator"""
    rng = np.random.default_rng(SEED)
    generic = R.draw_cases(rng, 2)                                                         # 8 counts x 7 times x 2 = 112
    zero = [R.draw_case(rng, cnt, 'inside', 'all_zero', il) for cnt, il in (((3, 5, 2, 7), True), ((16, 8, 4, 4), False))]
    infeasible = [infeasible_case(rng, cnt, il) for cnt, il in (((4, 4, 4, 4), True), ((16, 2, 2, 2), False), ((3, 5, 2, 7), True))]
    over = [overflow_case(rng, (17, 2, 2, 2)), overflow_case(rng, (16, 16, 2, 2))]
    A = generic + zero + infeasible
    # the same LP in other slots of the same batch: the tail of A repeats cases of its head, a 16-lane one among them
    twins = {}
    for src in range(5, len(generic), 10):
        if len(A) < B:
            twins[len(A)] = src; A.append(generic[src])
    assert len(A) == B
    # scale invariance: three feasible directions that take the entrywise check (at the normalised cost and, by preference, at 1e-2 of it too),
    # one of them with a 16-lane foot
    def qualifies(c, k):
        return c['ref']['feasible'] and np.abs(c['c']).max() > 0 and scaled(c, k)['nondegenerate']
    pool = [i for i, c in enumerate(generic) if qualifies(c, 0)]
    pool.sort(key=lambda i: not qualifies(generic[i], -2))
    wide = [i for i in pool if max(generic[i]['counts']) == 16][:1]
    dirs = wide + [i for i in pool if i not in wide and generic[i]['counts'] != generic[wide[0]]['counts']][:2]
    assert len(dirs) == 3
    Bb, scale_slots, ordinary = [], {}, {}
    for d in dirs:
        for k in SCALES:
            scale_slots[len(Bb)] = (d, k); Bb.append(scaled(generic[d], k))
    # capacity: the overflowing instances between ordinary ones (the first, one in the middle, the last slot), the ordinary ones being cases of A
    over_slots = {len(Bb): over[0], 77: over[1], B - 1: over[0]}
    src = 0
    while len(Bb) < B:
        if len(Bb) in over_slots:
            Bb.append(over_slots[len(Bb)])
        else:
            ordinary[len(Bb)] = src; Bb.append(A[src]); src += 1
    return A, Bb, dict(n_generic=len(generic), twins=twins, scale=scale_slots, ordinary=ordinary, over=sorted(over_slots), dirs=dirs)


def write_records(base, batch):
    """the cold start's records with nk, knot_kind, knot_time of every instance overwritten by its case's knot tables"""
    recs = (host.Trajectory * B).from_buffer_copy(bytes(base))
    for b, case in enumerate(batch):
        for ee in range(4):
            kk, tt = case['table'][ee]
            recs[b].nk[ee] = len(kk)
            for j in range(host.KMAX):
                recs[b].knot_kind[ee][j] = int(kk[j]) if j < len(kk) else 0
                recs[b].knot_time[ee][j] = float(tt[j]) if j < len(kk) else 0.0
    return recs


def solve_batch(g, gait, base, batch):
    g.set_warm_start_trajectory(write_records(base, batch))
    gait.set_contact_times_from_trajectory()
    xk, counts = gait.contact_times()
    grad = np.zeros((B, NV))
    for b, case in enumerate(batch):
        grad[b, :min(case['nv'], NV)] = case['c'][:NV]
    gait.set_gradient(grad, np.ones(B, np.int32))
    gait.optimize_contact_times(np.array([case['tnow'] for case in batch]))
    lp_status, pred = gait.lp_result()
    status, err = g.status()
    gg, valid = gait.gradient()
    return dict(xk=xk, counts=counts, lp_status=lp_status, pred=pred, step=gait.step(), err=err, grad_in=grad, grad_back=gg, valid=valid)


@functools.lru_cache(None)
def device():
    """both batches solved on one cold start"""
    A, Bb, _ = cases()
    cfg = load_config('a1_gait_opt_config', num_nodes=20, integrator_dt=0.05)
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * B, EE_NOMINAL)
    base = g.get_trajectory()
    gait = host.BatchGaitOptimizer(g)
    out = solve_batch(g, gait, base, A), solve_batch(g, gait, base, Bb)
    gait.close(); g.close()
    return out


def check_feasible(case, res, b):
    """every assertion on an LP the reference certifies feasible; returns (value error / E, entry error / bound or None)"""
    ref, nv, c = case['ref'], case['nv'], case['c']
    A_ub, b_ub, A_eq, b_eq = case['lp']
    x = res['step'][b, :nv]
    where = (b, case['counts'], case['time_how'], case['grad_how'], case.get('scale_k'))
    assert res['lp_status'][b] == 0, (where, res['lp_status'][b])
    pinned = R.pinned_columns(A_eq)
    assert np.all(x[pinned] == 0.0) and np.all(res['step'][b, nv:] == 0.0), where
    viol = (A_ub @ x - b_ub).max()
    assert viol <= 1e-9, (where, viol)
    val, E, tau = c @ x, case['E'], case['tau']
    print('  %s: value error %.2e of E = %.2e, row violation %.1e' % (where, abs(val - ref['f']) / E, E, max(viol, 0.0)), end='')
    assert abs(val - ref['f']) <= E, (where, val, ref['f'], E)
    assert abs(res['pred'][b] + val) <= 1e-9 * max(1.0, abs(val)), (where, res['pred'][b], val)
    slack = b_ub[case['rows']] - A_ub[case['rows']] @ x
    assert np.all(slack <= 2 * E / tau), (where, slack.max(), 2 * E / tau)
    entry = None
    if case['nondegenerate']:
        entry = np.abs(x - ref['x']).max() / (16 * 2 * E / tau)
        print(', entry error %.2e of the bound %.2e' % (entry, 16 * 2 * E / tau), end='')
        assert entry <= 1.0, (where, np.abs(x - ref['x']).max(), 16 * 2 * E / tau)
    print()
    return abs(val - ref['f']) / E, entry


def test_generator_meets_its_conditions():
    """at most 10 % of the draws infeasible (those built to be infeasible aside), at least 90 % of the feasible generic-gradient cases at a
    nondegenerate vertex -- the host-only twin of this test is in tests/test_lp_reference_host.py"""
    A, Bb, ix = cases()
    gen = A[:ix['n_generic']]
    feas = [c for c in gen if c['ref']['feasible']]
    assert len(gen) - len(feas) <= 0.1 * len(gen)
    plain = [c for c in feas if c['grad_how'] == 'generic']
    assert sum(c['nondegenerate'] for c in plain) >= 0.9 * len(plain)


@pytest.mark.parametrize('which', [0, 1], ids=['batch_a', 'batch_b'])
def test_written_schedules_come_back_bit_for_bit(which):
    batch, res = cases()[which], device()[which]
    for b, case in enumerate(batch):
        assert tuple(res['counts'][b]) == case['counts'], b
        want = np.zeros(NV)
        flat = np.concatenate(case['cts'])[:NV]
        want[:len(flat)] = flat
        same_bytes(res['xk'][b], want, 'contact times of instance %d' % b)
    same_bytes(res['grad_back'], res['grad_in'], 'gradient through srbm_gait_set_gradient')
    assert np.all(res['valid'] == 1)


def test_feasible_lps_match_the_exact_solver():
    A, _, ix = cases()
    res = device()[0]
    worst = {}
    for b in range(ix['n_generic'] + 2):                    # the drawn cases and the two with an all-zero gradient
        case = A[b]
        if not case['ref']['feasible']:
            assert res['lp_status'][b] != 0, b
            continue
        v, e = check_feasible(case, res, b)
        for fam in ('time ' + case['time_how'], 'gradient ' + case['grad_how'], 'counts ' + str(case['counts'])):
            w = worst.setdefault(fam, [0.0, 0.0])
            w[0] = max(w[0], v); w[1] = max(w[1], e or 0.0)
        if case['grad_how'] == 'all_zero':
            assert case['c'] @ res['step'][b, :case['nv']] == 0.0 and res['pred'][b] == 0.0
    for fam in sorted(worst):
        print('worst of %-28s value error / E %.2e   entry error / bound %.2e' % (fam, worst[fam][0], worst[fam][1]))


def test_infeasible_lps_are_reported_and_leave_their_neighbours_alone():
    A, _, ix = cases()
    res = device()[0]
    bad = [b for b in range(B) if A[b]['time_how'] == 'infeasible']
    assert len(bad) == 3
    for b in bad:
        assert not A[b]['ref']['feasible']
        assert res['lp_status'][b] != 0 and res['err'][b] == 0, (b, res['lp_status'][b], res['err'][b])
    # (their neighbours: every other instance of the batch is held to its reference above, and to its twin below)


def test_same_lp_in_another_slot_is_byte_equal():
    A, _, ix = cases()
    res = device()[0]
    assert len(ix['twins']) >= 8 and any(max(A[s]['counts']) == 16 for s in ix['twins'].values())
    for b, src in ix['twins'].items():
        for k in ('step', 'pred', 'lp_status'):
            same_bytes(res[k][b], res[k][src], '%s of instance %d against its twin %d' % (k, b, src))


def test_capacity_exits():
    """(17,2,2,2): a foot beyond its 16 lanes; (16,16,2,2): 36 contact times beyond the 32 of an instance.  Both are SRBM_ERR_CAPACITY with
    lp_status 2, no predicted reduction and a zero step, and the instances beside them are byte-equal to the same LPs solved in the batch
    without them."""
    A, Bb, ix = cases()
    ra, rb = device()
    assert len(ix['over']) == 3 and len(ix['ordinary']) >= 64
    for b in ix['over']:
        assert rb['err'][b] & ERR_CAPACITY, (b, rb['err'][b])
        assert rb['lp_status'][b] == 2 and rb['pred'][b] == 0.0 and np.all(rb['step'][b] == 0.0), b
    for b, src in ix['ordinary'].items():
        assert rb['err'][b] == 0, b
        for k in ('step', 'pred', 'lp_status'):
            same_bytes(rb[k][b], ra[k][src], '%s of instance %d beside an overflowing one against instance %d of the batch without' % (k, b, src))


def test_the_minimiser_does_not_depend_on_the_scale_of_the_cost():
    """three directions, |c|_inf = 10**k for k = -2 ... 12: solved at every k, to the same minimiser"""
    _, Bb, ix = cases()
    res = device()[1]
    failed, worst = [], {}
    for b, (d, k) in ix['scale'].items():
        case = Bb[b]
        print('direction %d %s, |c|_inf = 1e%d: lp_status %d' % (d, case['counts'], k, res['lp_status'][b]))
        if res['lp_status'][b] != 0:
            failed.append((d, k, int(res['lp_status'][b])))
            continue
        v, e = check_feasible(case, res, b)
        w = worst.setdefault(k, [0.0, 0.0])
        w[0] = max(w[0], v); w[1] = max(w[1], e or 0.0)
    for k in sorted(worst):
        print('worst at |c|_inf = 1e%-3d value error / E %.2e   entry error / bound %.2e' % (k, worst[k][0], worst[k][1]))
    assert not failed, 'not solved at (direction, k, lp_status): %s' % failed
