"""Rollout summaries on the device (include/srbm_rti.h: srbm_rollout_*; csrc/srbm_rollout_summary.hiph: srbm_k_rollout_fold, srbm_k_rollout_study;
through bilevel-gait-gen_amd/rollout_summary.py): the fold kernel, the host entry that compiles the same per-record fold and the per-record Python
restatement of tests/rollout_summary_kit.py give the SAME BYTES; chunking the rollout is invisible and needs a log of one chunk; summaries change no
result; the gait loop; the gather across ranks and the study record; the LARGE build; the refusals."""
import ctypes as C

import numpy as np
import pytest

import rollout_summary_kit as kit
from closed_loop_kit import GAIT_CASES, GAIT_FREQ, GAIT_RUNS, MODE, PUSH, SUB, assert_same, end_state, push_draw, rollout
from gpu_kit import same_bytes
from oracle_py import load_config
from srbm_loader import host, mpc_period, rollout_summary as rs
from srbm_loader.workloads import EE_NOMINAL, config_b_instance, instances

pytestmark = pytest.mark.gpu

B, STEPS, SUBSTEPS = 8, 12, 4          # 12 steps of 0.05 s: the default schedule switches contacts inside them (asserted below on the restatement)
LOWER_START = (0.0, 0.1)


def make_criteria(log, ref):
    """the settle radius and the momentum band are the medians of d2 and |h - h_ref|^2 over all records of the log itself; the other four are
    far from deciding anything on these rollouts but the fall height, which the pushed instances may cross"""
    r2, h2 = kit.medians_of_log(log, ref)
    return rs.criteria(z_min=0.2, tilt_max=0.5, r2_settle=r2, dz_settle=0.1, tilt_settle=0.1, h2_settle=h2)


def mu_of(g):
    return np.array([g.instance_model(b)[0].friction_coef for b in range(g.batch)])


@pytest.fixture(scope='module')
def base():
    """8 Config-B instances after their cold start, plant and pushes set, nothing run"""
    cfg = load_config()
    states, ees = instances(cfg, config_b_instance, B)
    pt, imp, _ = push_draw()
    g = host.BatchMPC.cold_start(cfg, states, ees, mode=LOWER_START)
    g.plant_set_state(states); g.plant_set_push(pt, imp)
    yield g
    g.close()


@pytest.fixture(scope='module')
def full(base):
    """the rollout with a 12-slot log folded in one call: (batch, log, criteria, ref, device summaries, closing snapshot), computed once"""
    g = base.clone()
    g.step_log_enable(STEPS)
    g.closed_loop_advance(0, STEPS, SUBSTEPS, True)
    log = g.step_log()
    ref = rs.reference_from_config(g.cfg, B)
    crit = make_criteria(log, ref)
    rs.enable(g, crit)                       # references: the tracking target of the configuration
    rs.fold(g)
    out = dict(g=g, log=log, crit=crit, ref=ref, summaries=rs.summaries(g), end=end_state(g))
    yield out
    g.close()


def test_device_equals_host_equals_restatement(full):
    log, crit, ref, dev = full['log'], full['crit'], full['ref'], full['summaries']
    mu = mu_of(full['g'])
    want = kit.fold(log, crit, ref, mu)
    F = rs.SUMMARY_FIELDS
    print('records in band per instance', want[:, 25], 'switches', want[:, 29], 'fallen at', want[:, 23], 'settled', rs.settled(want))
    # the case is not an empty one: records in and out of the band, a contact switch, every record counted
    assert (want[:, F['records']] == STEPS).all() and want[:, F['in_band']].sum() > 0 and (want[:, F['in_band']] < STEPS).any()
    assert (want[:, F['contact_switches']] > 0).any() and (want[:, F['nan_records']] == 0).all()
    assert (want[:, F['friction_margin_min']] < np.inf).all() and (want[:, F['iters_sum']] > 0).all()
    same_bytes(rs.fold_host(full['g'].L, log, crit, ref, mu), want, 'host entry against the restatement')
    same_bytes(dev, want, 'device summaries against the restatement')
    same_bytes(rs.summaries(full['g'], 3, 2), want[3:5], 'a range of instances')


def test_chunking_is_invisible_and_summaries_change_no_result(base, full):
    g = base.clone()
    g.step_log_enable(4)                      # one chunk
    rs.enable(g, full['crit'])
    for first in (0, 4, 8):                   # no synchronisation: launch, fold and cursor reset are ordered by the stream
        g.closed_loop_advance(first, 4, SUBSTEPS, True)
        rs.fold(g, 0, 4)
        g.step_log_reset()
    same_bytes(rs.summaries(g), full['summaries'], 'three chunks of 4 against one fold of 12')
    # ... and the module's driver, with a chunk that does not divide the steps
    d = base.clone()
    d.step_log_enable(5)
    rs.enable(d, full['crit'])
    rs.run(d, STEPS, 5, SUBSTEPS, True)
    same_bytes(rs.summaries(d), full['summaries'], 'run() in chunks of 5, 5, 2')
    assert d.step_log_count() == 0
    plain = base.clone()                      # never enabled summaries, never logged
    plain.closed_loop_advance(0, STEPS, SUBSTEPS, True)
    want = end_state(plain)
    assert_same(end_state(g), want, 'chunked with summaries against a plain rollout')
    assert_same(full['end'], want, 'logged and folded against a plain rollout')
    for x in (g, d, plain):
        x.close()


def test_gait_loop_in_chunks_of_one():
    cfgname, push_time, period = GAIT_CASES[0]
    cfg = load_config(cfgname)
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, EE_NOMINAL, mode=MODE)
    g.plant_set_state(s0); g.plant_set_push([push_time, 1e9], [PUSH, PUSH])            # the second instance is never pushed
    mpc_period.plant_set_period(g, period)
    twin = g.clone()
    tgait, troll = rollout(twin, log=GAIT_RUNS)
    troll.advance(1, GAIT_RUNS, GAIT_FREQ, SUB, True)
    log = twin.step_log()
    ref = rs.reference_from_config(cfg, 2)
    crit = make_criteria(log, ref)
    want = rs.fold_host(g.L, log, crit, ref, mu_of(g))
    gait, roll = rollout(g, log=1)
    rs.enable(g, crit)
    rs.run_gait(roll, GAIT_RUNS, 1, GAIT_FREQ, SUB, True)
    got = rs.summaries(g)
    same_bytes(got, want, 'gait loop in chunks of one run against the host fold of the fully logged twin')
    same_bytes(want, kit.fold(log, crit, ref, mu_of(g)), 'host fold against the restatement')
    kinds = log[:, :, 58]
    assert (got[:, 38] == (kinds == 1).sum(0)).all() and (got[:, 39] == (kinds == 2).sum(0)).all()
    assert (got[:, 38] > 0).all() and (got[:, 39] > 0).all() and (got[:, 0] == GAIT_RUNS).all()
    gait.close(); tgait.close(); g.close(); twin.close()


def test_gather_and_study(full):
    g, s = full['g'], full['summaries']
    hip = C.CDLL('libamdhip64.so')
    want = kit.study(s)
    same_bytes(rs.study(g), want, 'srbm_rollout_study against the restatement')
    same_bytes(rs.study_host(g.L, s), want, 'srbm_rollout_study_host against the restatement')
    assert want[0] == B
    comm = g.rccl_comm_init_rank(1, 0, g.rccl_unique_id())         # a world of one rank
    gathered, study = np.full((B, 64), -7.0), np.full(16, -7.0)
    p, q = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(gathered.nbytes)) == 0 and hip.hipMalloc(C.byref(q), C.c_size_t(study.nbytes)) == 0
    try:
        rs.allgather(g, comm, p.value)
        rs.study_dev(g, p.value, B, q.value)                        # queued behind the gather on the batch's stream
        g.synchronize()
        assert hip.hipMemcpy(gathered.ctypes.data_as(C.c_void_p), p, C.c_size_t(gathered.nbytes), 2) == 0       # hipMemcpyDeviceToHost
        assert hip.hipMemcpy(study.ctypes.data_as(C.c_void_p), q, C.c_size_t(study.nbytes), 2) == 0
    finally:
        hip.hipFree(p); hip.hipFree(q)
        g.rccl_comm_destroy(comm)
    same_bytes(gathered, s, 'the gathered array against the batch own summaries')
    same_bytes(study, want, 'study_dev on the gathered array against the restatement')


def test_large_build_long_horizon():
    cfg = load_config(num_nodes=80, integrator_dt=0.02)
    s0 = np.array(cfg['srb_init'], float)
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, EE_NOMINAL, mode=MODE, large=True)
    assert g.large
    g.plant_set_state(s0); g.plant_set_push([0.03, 1e9], [PUSH, PUSH])
    g.step_log_enable(3)
    g.closed_loop_advance(0, 3, SUBSTEPS, True)
    log = g.step_log()
    ref = rs.reference_from_config(cfg, 2)
    crit = make_criteria(log, ref)
    rs.enable(g, crit)
    rs.fold(g)
    want = rs.fold_host(g.L, log, crit, ref, mu_of(g))
    assert (want[:, 0] == 3).all() and (want[:, 1] == log[0, :, 0]).all()
    same_bytes(rs.summaries(g), want, 'LARGE build: device summaries against the host fold')
    g.close()


def test_refusals_on_the_device_path(base, full):
    g = base.clone()
    assert g.L.srbm_rollout_summary_get(g.h, 0, 1, np.zeros(64).ctypes.data_as(C.POINTER(C.c_double))) != 0        # a clone has summaries off
    with pytest.raises(RuntimeError, match='no step log'):
        rs.fold(g, 0, 0)                                                            # before a log exists
    g.step_log_enable(4)
    with pytest.raises(RuntimeError, match='no rollout summary'):
        rs.fold(g, 0, 0)                                                            # before enable
    for bad in (dict(z_min=np.nan), dict(h2_settle=np.inf)):
        with pytest.raises(RuntimeError, match='not finite'):
            rs.enable(g, rs.criteria(**dict(dict(z_min=0.2, tilt_max=0.5, r2_settle=1.0, dz_settle=0.1, tilt_settle=0.1, h2_settle=1.0), **bad)))
    c = full['crit'].copy(); c[7] = 1.0
    with pytest.raises(RuntimeError, match='reserved'):
        rs.enable(g, c)
    with pytest.raises(RuntimeError, match='no rollout summary'):
        rs.summaries(g)                                                             # the refused enables left them off
    rs.enable(g, full['crit'])
    g.closed_loop_advance(0, 2, SUBSTEPS, True)
    rs.fold(g, 0, 2)
    before = rs.summaries(g)
    assert (before[:, 0] == 2).all()
    for first, count in ((0, 3), (2, 1), (-1, 1), (0, -1), (3, 0)):                 # past the cursor (2 of 4 slots logged)
        with pytest.raises(RuntimeError, match='outside'):
            rs.fold(g, first, count)
    with pytest.raises(RuntimeError, match='outside'):
        rs.summaries(g, 7, 2)
    same_bytes(rs.summaries(g), before, 'the summaries after the refused calls')
    rs.reset(g)
    same_bytes(rs.summaries(g), rs.empty(B), 'the summaries after a reset')
    cl = g.clone()
    with pytest.raises(RuntimeError, match='no rollout summary'):
        rs.summaries(cl)                                                            # a clone has summaries off, as it has logging off
    rs.enable(g, None)
    with pytest.raises(RuntimeError, match='no rollout summary'):
        rs.study(g)
    cl.close(); g.close()
