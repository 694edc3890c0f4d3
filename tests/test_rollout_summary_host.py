"""Rollout summaries without a GPU (include/srbm_rti.h: srbm_rollout_fold_host, srbm_rollout_study_host -- the per-record fold and the study reduction
the kernels of csrc/srbm_rollout_summary.hiph run, compiled for the host) against the restatement of tests/rollout_summary_kit.py, bit for bit, in
both builds of the library."""
import ctypes as C

import numpy as np
import pytest

import rollout_summary_kit as kit
from gpu_kit import same_bytes
from srbm_loader import host, rollout_summary as rs

DP = C.POINTER(C.c_double)
F = rs.SUMMARY_FIELDS


@pytest.fixture(scope='module', params=[False, True], ids=['standard', 'large'])
def L(request):
    host.build()
    return host.lib(request.param)


@pytest.fixture(scope='module')
def synth():
    """the synthetic log and the restatement's summaries of it, computed once"""
    log = kit.synthetic_log()
    return log, kit.fold(log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU)


def test_summary_size_without_a_gpu(L):
    assert L.srbm_rollout_summary_doubles() == 64 == rs.SUMMARY_DOUBLES


def test_field_tables_tile_the_records():
    for table, end in ((rs.SUMMARY_FIELDS, 43), (rs.STUDY_FIELDS, 11)):
        hits = np.zeros(end, int)
        for sl in table.values():
            assert 0 <= sl.start < sl.stop <= end and sl.step is None
            hits[sl] += 1
        assert (hits == 1).all(), hits
    same_bytes(rs.empty(3), np.array([kit.empty_summary()] * 3), 'the reset state')


def test_the_events_are_in_the_restatement(synth):
    """every event the synthetic log was given shows in the restatement's summaries: the comparison below cannot pass on an empty case"""
    _, s = synth
    assert (s[:, 0] == 9).all() and (s[:, 1] == 11).all() and (s[:, 2] == 19).all() and (s[:, 43:] == 0).all()
    same_bytes(s[:, 3], np.full(5, 0.05 * 1), 'first init_time'); same_bytes(s[:, 4], np.full(5, 0.05 * 9), 'last init_time')
    # instance 0: fall by height at 3; statuses 1 and 3; error bits on two records
    assert s[0, 23] == 3 and s[0, 15] == 0.1 and list(s[0, 5:9]) == [2, 2, 1, 130]
    # instance 1: fall by tilt at 6; one NaN record; foot 3 never in contact and the margin from the other feet
    assert s[1, 23] == 6 and s[1, 19] == 0.72 and s[1, 20] == 6 and s[1, 28] == 1 and s[1, 29] == 0
    assert list(s[1, 34:38]) == [8, 8, 8, 0] and 0 < s[1, 27] < np.inf and list(s[1, 30:34]) == [1, 1, 1, 0]
    assert (s[[0, 2, 3, 4], 28] == 0).all() and (s[[2, 3, 4], 23] == -1).all() and (s[1:, 5:9] == [0, -1, 0, 0]).all()
    # instance 2: equal maxima, the first keeps the ordinal; two contact switches
    assert s[2, 18] == 2 and s[2, 20] == 1 and s[2, 19] == 0.125 and s[2, 29] == 2 and list(s[2, 30:38]) == [0, 0, 1, 1, 3, 6, 9, 9]
    # instance 3: gait kinds 1 and 2 with imin 0 and 3; ends in band from record 6 on
    assert list(s[3, 38:43]) == [2, 2, 0.75, 1, 0.0075] and s[3, 24] == 5 and s[3, 25] == 3 and (s[[0, 1, 2, 4], 38:43] == 0).all()
    # instance 4: leaves the band on its last record
    assert s[4, 24] == 8 and s[4, 25] == 8 and s[4, 21] > 4.0
    assert list(rs.settled(s)) == [False, False, True, True, False]
    assert (s[:, 9] >= 9 * 8).all() and (s[:, 10] <= 24).all() and (s[:, 13] >= 0.5).all() and (s[:, 26] > 20).all() and (s[:, 16] > s[:, 15]).all()


def test_fold_host_is_the_restatement_bit_for_bit(L, synth):
    log, want = synth
    got = rs.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU)
    same_bytes(got, want, 'srbm_rollout_fold_host against the restatement')


def test_chunking_is_invisible_and_zero_records_change_nothing(L, synth):
    log, want = synth
    a = rs.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU, first_slot=0, count=4)
    same_bytes(a, kit.fold(log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU, count=4), 'slots [0, 4)')
    b = rs.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU, into=a, first_slot=4, count=5)
    same_bytes(b, want, '[0, 4) then [4, 9) against [0, 9)')
    for first in (0, 4, 9):
        same_bytes(rs.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU, into=a, first_slot=first, count=0), a, 'zero records from %d' % first)
    same_bytes(rs.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, kit.SYNTH_MU, count=0), rs.empty(5), 'zero records into the reset state')


def test_study_host_is_the_restatement(L, synth):
    _, s = synth
    want = kit.study(s)
    same_bytes(rs.study_host(L, s), want, 'srbm_rollout_study_host against the restatement')
    T = rs.STUDY_FIELDS
    n, fallen, settled, failed = (want[T[k]][0] for k in ('instances', 'fallen', 'settled', 'failed'))
    assert n == 5 and (fallen, settled, failed) == (2, 2, 1)                 # all non-zero, all below the number of instances
    assert want[4] == 6 and want[5] == 12 and want[6] == s[:, 17].max() and want[7] == 0.72 and want[8] == s[:, 27].min() and want[10] == 130
    assert want[9] == s[:, 9].sum() and (want[11:] == 0).all()
    # instance order and a partial array: the study of the first two instances has nobody settled
    two = kit.study(s[:2])
    same_bytes(rs.study_host(L, s[:2]), two, 'two instances')
    assert two[2] == 0 and two[4] == -1 and two[5] == 0
    same_bytes(rs.study_host(L, s[:0]), kit.study(s[:0]), 'no instance')


def test_refusals_leave_the_output_untouched(L, synth):
    log, _ = synth
    d = lambda a: a.ctypes.data_as(DP)
    crit, ref, mu = kit.SYNTH_CRIT.copy(), np.ascontiguousarray(kit.SYNTH_REF), kit.SYNTH_MU.copy()
    out = rs.empty(5); out[:, 43] = 7.0
    before = out.copy()

    def refused(words, log_=log, slots=9, batch=5, first=0, count=9, crit_=crit, ref_=ref, mu_=mu, out_=out):
        rc = L.srbm_rollout_fold_host(None if log_ is None else d(log_), slots, batch, first, count, None if crit_ is None else d(crit_),
                                      None if ref_ is None else d(ref_), None if mu_ is None else d(mu_), None if out_ is None else d(out_))
        assert rc != 0, words
        assert words in L.srbm_last_error().decode(), (words, L.srbm_last_error())
        same_bytes(out, before, 'the summaries after a refusal (%s)' % words)

    refused('outside', first=5, count=5)
    refused('outside', first=-1, count=2)
    refused('outside', first=0, count=-1)
    refused('outside', first=10, count=0)
    for nul in ('log_', 'crit_', 'ref_', 'mu_', 'out_'):
        refused('bad arguments', **{nul: None})
    refused('bad arguments', batch=0)
    for i, v in ((0, np.nan), (2, np.inf), (5, -np.inf)):
        c = crit.copy(); c[i] = v
        refused('criterion %d is not finite' % i, crit_=c)
    for i in (6, 7):
        c = crit.copy(); c[i] = 1e-300
        refused('criterion %d is reserved' % i, crit_=c)
    study = np.full(16, 7.0)
    assert L.srbm_rollout_study_host(None, 5, d(study)) != 0 and L.srbm_rollout_study_host(d(out), -1, d(study)) != 0
    assert L.srbm_rollout_study_host(d(out), 5, None) != 0 and 'bad arguments' in L.srbm_last_error().decode()
    assert (study == 7.0).all()
    # the module refuses a criteria array of another length before the library is called
    with pytest.raises(ValueError):
        rs.fold_host(L, log, crit[:6], ref, mu)
