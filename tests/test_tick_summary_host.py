"""Tick summaries without a GPU (include/srbm_rti.h: srbm_tick_fold_host, srbm_tick_study_host -- the per-record fold and the study reduction the
kernels of csrc/srbm_tick_summary.hiph run, compiled for the host) against the restatement of tests/tick_summary_kit.py, bit for bit, in both builds
of the library."""
import ctypes as C

import numpy as np
import pytest

import tick_summary_kit as kit
from gpu_kit import same_bytes
from srbm_loader import host, tick_summary as ts

DP = C.POINTER(C.c_double)
F = ts.SUMMARY_FIELDS
N, NB = kit.SYNTH_SLOTS, kit.SYNTH_BATCH


@pytest.fixture(scope='module', params=[False, True], ids=['standard', 'large'])
def L(request):
    host.build()
    return host.lib(request.param)


@pytest.fixture(scope='module')
def synth():
    """the synthetic log and the restatement's summaries of it, computed once"""
    log = kit.synthetic_log()
    return log, kit.fold(log, kit.SYNTH_CRIT, kit.SYNTH_REF)


def test_summary_size_without_a_gpu(L):
    assert L.srbm_tick_summary_doubles() == 64 == ts.SUMMARY_DOUBLES


def test_field_tables_tile_the_records():
    for table, end in ((ts.SUMMARY_FIELDS, 62), (ts.STUDY_FIELDS, 16)):
        hits = np.zeros(end, int)
        for sl in table.values():
            assert 0 <= sl.start < sl.stop <= end and sl.step is None
            hits[sl] += 1
        assert (hits == 1).all(), hits
    same_bytes(ts.empty(3), np.array([kit.empty_summary()] * 3), 'the reset state')


def test_the_events_are_in_the_restatement(synth):
    """every event the synthetic log was given shows in the restatement's summaries, each value stated by hand: the bitwise comparisons below cannot
    pass on an empty case"""
    log, t = synth
    assert (t[:, 0] == N).all() and (t[:, 1] == 100).all() and (t[:, 2] == 109).all() and (t[:, 62:] == 0).all() and (t[:, 42] == 0).all()
    same_bytes(t[:, 3], np.full(NB, 0.001 * 100), 'first time'); same_bytes(t[:, 4], np.full(NB, 0.001 * 109), 'last time')
    # instance 0: fall by height at 3; targets status 1 and 2; QP status 8 with the coast flag at 6; pushes at 1 and 4 (the LAST keeps the
    # ordinal), updates after 4 and 9; -3 and 2^53 in field 5 set no bit
    assert t[0, 24] == 3 and t[0, 16] == 0.1 and list(t[0, 5:9]) == [2, 2, 1, 6] and list(t[0, 11:16]) == [2, 4, 2, 1, 0]
    # a kind-0 instance: fields 43..61 stay at reset
    for b in (0, 2, 4, 5):
        same_bytes(t[b, 43:62], ts.empty(1)[0, 43:62], 'fields 43..61 of instance %d' % b)
    assert (t[1:, 5:9] == [0, -1, 0, -1]).all() and (t[[2, 3, 4, 5], 11:16] == [0, -1, 0, 0, 0]).all()
    # instance 1: fall by tilt at 6; one NaN record, whose flag bit 3 counts and whose field 60 does not; clamped joints 2 + 3 on two records;
    # the held feet pull on two records, hardest with -1.5; no ground; foot 3 never in desired contact
    assert t[1, 24] == 6 and t[1, 20] == 0.72 and t[1, 21] == 6 and t[1, 31] == 1 and list(t[1, 11:16]) == [0, -1, 0, 0, 1]
    assert list(t[1, 43:46]) == [9, 2, 5] and t[1, 47] == -1.5 and t[1, 48] == 2 and t[1, 46] == np.delete(log[:, 1, 59], 4).max()
    assert list(t[1, 51:62]) == [0, 0, 0, 0, 0, 0, 0, 0, -1, 0, -1] and t[1, 32] == 0
    assert list(t[1, 33:41]) == [1, 1, 1, 0, 9, 9, 9, 0] and t[1, 41] == 0.05 + 0.003 * 9 and t[1, 30] < 0.002
    assert (t[[0, 2, 3, 4, 5], 31] == 0).all() and (t[[2, 3, 4, 5], 24] == -1).all() and (t[[0, 3, 4, 5], 41] == -np.inf).all()
    # instance 2: equal maxima, the first keeps the ordinal; two desired-contact switches; out of band last at 7
    assert t[2, 19] == 2 and t[2, 21] == 1 and t[2, 20] == 0.125 and t[2, 32] == 2 and list(t[2, 33:41]) == [0, 0, 1, 1, 3, 6, 10, 10]
    dx = log[2, 2, 6] - kit.SYNTH_REF[2, 0]
    assert t[2, 41] == max(log[3:, 2, 47].max(), log[6:, 2, 48].max()) and t[2, 18] == dx * dx and log[7, 2, 6] == log[2, 2, 6] and t[2, 25] == 7 and t[2, 26] == 6
    # instance 3: on a ground.  Contacts 15 x 5, 0, 11 x 4; slip bits 1 + 2 + 1, first at 2; mismatch bits 4 + 1; airborne once; two switches
    assert list(t[3, 51:62]) == [10, 9, 9, 5, 9, 4, 5, 1, 2, 2, 11] and list(t[3, 43:46]) == [10, 1, 1] and t[3, 48] == 0 and t[3, 47] >= 5.0
    assert t[3, 25] == -1 and t[3, 26] == 10
    # instance 4: ends in band from record 6 on; a NaN in field 5 sets no bit and makes no NaN record
    assert t[4, 25] == 5 and t[4, 26] == 4 and t[4, 31] == 0
    # instance 5: leaves the band on its last record; no field 63 of it is a ground word
    assert t[5, 25] == 9 and t[5, 26] == 9 and t[5, 22] > 8.0 and t[5, 51] == 0
    assert list(ts.settled(t)) == [False, False, True, True, True, False]
    assert (t[:, 9] >= 3 * N).all() and (t[:, 10] <= 12).all() and (t[:, 29] > 20).all() and (t[:, 17] > t[:, 16]).all()
    assert (t[:, 27] <= 10).all() and (t[:, 27] > 5).all() and (t[:, 28] > 0).all() and (t[:, 23] > 0).all()


def test_fold_host_is_the_restatement_bit_for_bit(L, synth):
    log, want = synth
    got = ts.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF)
    same_bytes(got, want, 'srbm_tick_fold_host against the restatement')


def test_chunking_is_invisible_and_zero_records_change_nothing(L, synth):
    log, want = synth
    a = ts.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, first_slot=0, count=4)
    same_bytes(a, kit.fold(log, kit.SYNTH_CRIT, kit.SYNTH_REF, count=4), 'slots [0, 4)')
    b = ts.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, into=a, first_slot=4, count=6)
    same_bytes(b, want, '[0, 4) then [4, 10) against [0, 10)')
    for first in (0, 4, 10):
        same_bytes(ts.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, into=a, first_slot=first, count=0), a, 'zero records from %d' % first)
    same_bytes(ts.fold_host(L, log, kit.SYNTH_CRIT, kit.SYNTH_REF, count=0), ts.empty(NB), 'zero records into the reset state')


def test_study_host_is_the_restatement(L, synth):
    _, t = synth
    want = kit.study(t)
    same_bytes(ts.study_host(L, t), want, 'srbm_tick_study_host against the restatement')
    U = ts.STUDY_FIELDS
    n, fallen, settled, zero = (want[U[k]][0] for k in ('instances', 'fallen', 'settled', 'zero_action'))
    assert n == NB and (fallen, settled, zero) == (2, 3, 1)
    assert want[4] == 8 and want[5] == 8 + 0 + 6 and want[6] == t[:, 18].max() and want[7] == 0.72 and want[8] == t[:, 27].max()
    assert want[9] == t[:, 9].sum() and list(want[10:15]) == [3, 1, 4, 5, 1] and want[15] == -1.5
    # instance order and a partial array: the study of the first two instances has nobody settled and no ground
    two = kit.study(t[:2])
    same_bytes(ts.study_host(L, t[:2]), two, 'two instances')
    assert two[2] == 0 and two[4] == -1 and two[5] == 0 and two[12] == 0
    same_bytes(ts.study_host(L, t[:0]), kit.study(t[:0]), 'no instance')


def test_refusals_leave_the_output_untouched(L, synth):
    log, _ = synth
    d = lambda a: a.ctypes.data_as(DP)
    crit, ref = kit.SYNTH_CRIT.copy(), np.ascontiguousarray(kit.SYNTH_REF)
    out = ts.empty(NB); out[:, 62] = 7.0
    before = out.copy()

    def refused(words, log_=log, slots=N, batch=NB, first=0, count=N, crit_=crit, ref_=ref, out_=out):
        rc = L.srbm_tick_fold_host(None if log_ is None else d(log_), slots, batch, first, count, None if crit_ is None else d(crit_),
                                   None if ref_ is None else d(ref_), None if out_ is None else d(out_))
        assert rc != 0, words
        assert words in L.srbm_last_error().decode(), (words, L.srbm_last_error())
        assert 'srbm_tick_fold_host' in L.srbm_last_error().decode()
        same_bytes(out, before, 'the summaries after a refusal (%s)' % words)

    refused('outside', first=5, count=6)
    refused('outside', first=-1, count=2)
    refused('outside', first=0, count=-1)
    refused('outside', first=11, count=0)
    for nul in ('log_', 'crit_', 'ref_', 'out_'):
        refused('bad arguments', **{nul: None})
    refused('bad arguments', batch=0)
    refused('bad arguments', slots=-1)
    for i, v in ((0, np.nan), (2, np.inf), (5, -np.inf)):
        c = crit.copy(); c[i] = v
        refused('criterion %d is not finite' % i, crit_=c)
    for i in (6, 7):
        c = crit.copy(); c[i] = 1e-300
        refused('criterion %d is reserved' % i, crit_=c)
    study = np.full(16, 7.0)
    assert L.srbm_tick_study_host(None, NB, d(study)) != 0 and L.srbm_tick_study_host(d(out), -1, d(study)) != 0
    assert L.srbm_tick_study_host(d(out), NB, None) != 0 and 'srbm_tick_study_host: bad arguments' in L.srbm_last_error().decode()
    assert (study == 7.0).all()
    # the module refuses a criteria array of another length, and references of another shape, before the library is called
    with pytest.raises(ValueError):
        ts.fold_host(L, log, crit[:6], ref)
    with pytest.raises(ValueError):
        ts.fold_host(L, log, crit, ref[:, :5])
