"""Rollout summaries (include/srbm_rti.h: srbm_rollout_*; csrc/srbm_rollout_summary.hiph): the step log of a closed-loop rollout folded on the device
into one outcome record of 64 doubles per instance -- fallen, settled from, worst deviation, friction margin, failed solves -- and the summaries of a
batch, or of all ranks after a gather, reduced to one study record of 16 doubles.  The fold is incremental: log a chunk of steps, fold it, reset the log
cursor, repeat; a rollout of any length needs a log of one chunk, and the summaries do not depend on the chunking, bit for bit.  A module of its own
beside host.py, as gait_rollout.py and mpc_period.py are: it calls through the library `host.declare` has typed.

    crit = criteria(z_min=0.15, tilt_max=0.5, r2_settle=0.02 ** 2, dz_settle=0.02, tilt_settle=0.01, h2_settle=0.5 ** 2)
    mpc.step_log_enable(chunk); enable(mpc, crit)            references: the tracking target of the configuration
    run(mpc, steps, chunk, substeps, advance_time)           closed_loop_advance(chunk) -> fold -> step_log_reset, ONE synchronisation at the end
    S = summaries(mpc); settled(S); study(mpc)               S[:, SUMMARY_FIELDS['first_fallen']], study(mpc)[STUDY_FIELDS['settled']]
"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)
SUMMARY_DOUBLES, CRITERIA_DOUBLES, REF_DOUBLES, STUDY_DOUBLES = 64, 8, 6, 16

# one summary: field name -> slice of its 64 doubles ([43, 64) is 0); ordinals count the records folded since the last reset from 0, -1: none
SUMMARY_FIELDS = {
    'records': slice(0, 1), 'first_solve': slice(1, 2), 'last_solve': slice(2, 3), 'first_time': slice(3, 4), 'last_time': slice(4, 5),
    'not_solved': slice(5, 6), 'first_not_solved': slice(6, 7), 'failed': slice(7, 8), 'err': slice(8, 9), 'iters_sum': slice(9, 10),
    'iters_max': slice(10, 11), 'cost_sum': slice(11, 12), 'defect_max': slice(12, 13), 'alpha_min': slice(13, 14), 'step_norm_max': slice(14, 15),
    'z_min': slice(15, 16), 'z_max': slice(16, 17), 'd2_max': slice(17, 18), 'd2_max_at': slice(18, 19), 'tilt_max': slice(19, 20),
    'tilt_max_at': slice(20, 21), 'h2_max': slice(21, 22), 'L2_max': slice(22, 23), 'first_fallen': slice(23, 24), 'last_out_of_band': slice(24, 25),
    'in_band': slice(25, 26), 'fz_max': slice(26, 27), 'friction_margin_min': slice(27, 28), 'nan_records': slice(28, 29),
    'contact_switches': slice(29, 30), 'last_flags': slice(30, 34), 'contact_count': slice(34, 38), 'gradient_runs': slice(38, 39),
    'line_search_runs': slice(39, 40), 'pred_red_sum': slice(40, 41), 'line_search_moved': slice(41, 42), 'last_winner_cost': slice(42, 43)}
# one study record: [11, 16) is 0
STUDY_FIELDS = {
    'instances': slice(0, 1), 'fallen': slice(1, 2), 'settled': slice(2, 3), 'failed': slice(3, 4), 'settled_from_max': slice(4, 5),
    'settled_from_sum': slice(5, 6), 'd2_max': slice(6, 7), 'tilt_max': slice(7, 8), 'friction_margin_min': slice(8, 9), 'iters_sum': slice(9, 10),
    'err': slice(10, 11)}


def criteria(z_min, tilt_max, r2_settle, dz_settle, tilt_settle, h2_settle):
    """criteria[8]: fallen if p_z < z_min or u > tilt_max; in band if d2 <= r2_settle, |p_z - ref_z| <= dz_settle, u <= tilt_settle and
    |h - h_ref|^2 <= h2_settle.  Squared quantities: d2 and h2 are squared norms, u = 2 (qx^2 + qy^2) = 1 - cos(tilt); the two reserved entries are 0"""
    return np.array([z_min, tilt_max, r2_settle, dz_settle, tilt_settle, h2_settle, 0.0, 0.0], dtype=np.float64)


def empty(instances):
    """summaries[instances][64] in the state after a reset (what the host fold starts from): counts and sums 0, maxima -inf, minima +inf, ordinals -1"""
    s = np.zeros((int(instances), SUMMARY_DOUBLES))
    s[:, [6, 18, 20, 23, 24]] = -1.0
    s[:, [10, 12, 14, 16, 17, 19, 21, 22, 26]] = -np.inf
    s[:, [13, 15, 27]] = np.inf
    return s


def _criteria_array(crit):
    a = np.ascontiguousarray(crit, dtype=np.float64)
    if a.shape != (CRITERIA_DOUBLES,):
        raise ValueError('criteria: %d doubles expected (criteria(...)), got shape %s' % (CRITERIA_DOUBLES, a.shape))
    return a


def reference_from_config(cfg, batch):
    """ref[batch][6]: position and linear momentum of the configuration's tracking target (srb_target: p, h, quaternion, L)"""
    t = np.asarray(cfg['srb_target'], dtype=np.float64)
    return np.tile(t[:REF_DOUBLES], (batch, 1))


def enable(mpc, crit, ref=None):
    """allocate and reset the summaries of the batch; crit: criteria(...); ref: [6] for the whole batch or [batch][6] = {p_ref, h_ref}, None: the
    tracking target of the batch's configuration.  crit None: summaries off, buffers freed"""
    if crit is None:
        mpc._chk(mpc.L.srbm_rollout_summary_enable(mpc.h, None, None))
        return
    r = reference_from_config(mpc.cfg, mpc.batch) if ref is None else np.asarray(ref, dtype=np.float64)
    if r.shape == (REF_DOUBLES,):
        r = np.tile(r, (mpc.batch, 1))
    if r.shape != (mpc.batch, REF_DOUBLES):
        raise ValueError('ref: shape (%d,) or (%d, %d) expected, got %s' % (REF_DOUBLES, mpc.batch, REF_DOUBLES, r.shape))
    r = np.ascontiguousarray(r)
    mpc._chk(mpc.L.srbm_rollout_summary_enable(mpc.h, _criteria_array(crit).ctypes.data_as(_dp), r.ctypes.data_as(_dp)))


def reset(mpc):
    """the summaries back to the state of empty(); asynchronous on the batch's stream"""
    mpc._chk(mpc.L.srbm_rollout_summary_reset(mpc.h))


def fold(mpc, first_slot=0, count=None):
    """fold the log slots [first_slot, first_slot + count) (None: up to the cursor) into the summaries; asynchronous on the batch's stream"""
    count = mpc.step_log_count() - first_slot if count is None else count
    mpc._chk(mpc.L.srbm_rollout_summary_fold(mpc.h, int(first_slot), int(count)))


def summaries(mpc, first=0, count=None):
    """summaries[count][64] of instances [first, first + count); synchronous"""
    count = mpc.batch - first if count is None else count
    out = np.zeros((max(int(count), 0), SUMMARY_DOUBLES))
    mpc._chk(mpc.L.srbm_rollout_summary_get(mpc.h, int(first), int(count), out.ctypes.data_as(_dp)))
    return out


def study(mpc):
    """the study record [16] of the batch's own summaries; synchronous"""
    out = np.zeros(STUDY_DOUBLES)
    mpc._chk(mpc.L.srbm_rollout_study(mpc.h, out.ctypes.data_as(_dp)))
    return out


def study_dev(mpc, summaries_ptr, instances, study_ptr):
    """the study record of summaries[instances][64] at device address summaries_ptr (a gathered array) into device memory at study_ptr ([16]), on the
    batch's stream, no synchronisation"""
    mpc._chk(mpc.L.srbm_rollout_study_dev(mpc.h, summaries_ptr, int(instances), study_ptr))


def allgather(mpc, comm, out_ptr):
    """this rank's summaries into their slot of out[world * batch][64] (device pointer) and ONE in-place ncclAllGather on the batch's stream; comm as
    BatchMPC.rccl_comm_init_rank returns it; asynchronous"""
    mpc._chk(mpc.L.srbm_rollout_allgather_dev(mpc.h, comm, out_ptr))


def settled(s):
    """bool[instances]: the instance did not fall and its last record is in band (field 23 < 0 and field 24 < field 0 - 1); settled from = field 24 + 1"""
    s = np.asarray(s, dtype=np.float64).reshape(-1, SUMMARY_DOUBLES)
    return (s[:, 23] < 0) & (s[:, 24] < s[:, 0] - 1)


# ---- the same fold and reduction on the host (no GPU, no batch) ----
def fold_host(L, log, crit, ref, mu, into=None, first_slot=0, count=None):
    """L: a loaded library (host.lib()); log[slots][batch][64]; ref[batch][6]; mu[batch]; into: summaries[batch][64] to continue (None: empty()).
    Returns the summaries after folding the slots [first_slot, first_slot + count) in ascending order"""
    log = np.ascontiguousarray(log, dtype=np.float64)
    slots, batch = log.shape[0], log.shape[1]
    count = slots - first_slot if count is None else count
    out = empty(batch) if into is None else np.array(into, dtype=np.float64).reshape(batch, SUMMARY_DOUBLES)
    ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(batch, REF_DOUBLES)
    mu = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (batch,)))
    rc = L.srbm_rollout_fold_host(log.ctypes.data_as(_dp), slots, batch, int(first_slot), int(count), _criteria_array(crit).ctypes.data_as(_dp),
                                  ref.ctypes.data_as(_dp), mu.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return out


def study_host(L, s):
    """the study record [16] of summaries[instances][64], instances in ascending order"""
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1, SUMMARY_DOUBLES)
    out = np.zeros(STUDY_DOUBLES)
    if L.srbm_rollout_study_host(s.ctypes.data_as(_dp), len(s), out.ctypes.data_as(_dp)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return out


# ---- the chunked drivers ----
def _chunks(first, steps, chunk):
    if chunk < 1:
        raise ValueError('chunk: at least one step')
    done = 0
    while done < steps:
        n = min(chunk, steps - done)
        yield first + done, n
        done += n


def run(mpc, steps, chunk, substeps, advance_time, first_index=0):
    """closed-loop iterations first_index .. first_index + steps - 1 in launches of `chunk` steps: cursor to 0, closed_loop_advance, fold -- all queued
    on the batch's stream, ONE synchronisation at the end.  The step log needs room for one chunk only (step_log_enable(chunk)); whatever it held
    before is overwritten"""
    for first, n in _chunks(first_index, steps, chunk):
        mpc.step_log_reset()
        mpc.closed_loop_advance(first, n, substeps, advance_time)
        fold(mpc, 0, n)
    mpc.step_log_reset()
    mpc.synchronize()


def run_gait(roll, runs, chunk, gait_opt_freq, substeps, advance_time, first_run_num=1):
    """the same driver for gait_rollout.GaitRollout: runs first_run_num .. first_run_num + runs - 1 of the gait loop closed over the plant"""
    mpc = roll.mpc
    for first, n in _chunks(first_run_num, runs, chunk):
        mpc.step_log_reset()
        roll.advance(first, n, gait_opt_freq, substeps, advance_time)
        fold(mpc, 0, n)
    mpc.step_log_reset()
    mpc.synchronize()
