"""Tick summaries (include/srbm_rti.h: srbm_tick_summary_*, srbm_tick_study*; csrc/srbm_tick_summary.hiph): the tick log of a whole-controller rollout
folded on the device into one outcome record of 64 doubles per instance -- fallen, settled from, torque peaks, clamped joints, a held foot that pulls,
slipping feet, the plan against the ground -- and the summaries of a batch, or of all ranks after a gather, reduced to one study record of 16 doubles.
The tick-level counterpart of rollout_summary.py, which folds the step log (one record per MPC update): the same entries, the same refusals.  The fold
is incremental: log a chunk of ticks, fold it, reset the log cursor, repeat; a rollout of any length needs a tick log of one chunk, and the summaries
do not depend on the chunking, bit for bit.  A module of its own beside host.py: it calls through the library `host.declare` has typed.

    crit = criteria(z_min=0.15, tilt_max=0.5, r2_settle=0.02 ** 2, dz_settle=0.02, tilt_settle=0.01, v2_settle=0.1 ** 2)
    R.tick_log_enable(chunk); enable(mpc, crit, ref)         R: controller_rollout.ControllerRollout(mpc); ref[batch][6] = {p_ref, v_ref}
    run(R, ticks, chunk, ticks_per_update, tick_dt)          cursor 0 -> R.advance(chunk) -> fold, ONE synchronisation at the end
    T = summaries(mpc); settled(T); study(mpc)               T[:, SUMMARY_FIELDS['first_fallen']], study(mpc)[STUDY_FIELDS['pulling']]
"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)
SUMMARY_DOUBLES, CRITERIA_DOUBLES, REF_DOUBLES, STUDY_DOUBLES, TICK_LOG_DOUBLES = 64, 8, 6, 16, 64

# one summary: field name -> slice of its 64 doubles ([62, 64) is 0, and so is field 42); ordinals count the records folded since the last reset
# from 0, -1: none
SUMMARY_FIELDS = {
    'records': slice(0, 1), 'first_tick': slice(1, 2), 'last_tick': slice(2, 3), 'first_time': slice(3, 4), 'last_time': slice(4, 5),
    'targets_failed': slice(5, 6), 'first_targets_failed': slice(6, 7), 'zero_action': slice(7, 8), 'first_zero_action': slice(8, 9),
    'qp_iters_sum': slice(9, 10), 'qp_iters_max': slice(10, 11), 'pushed': slice(11, 12), 'last_pushed': slice(12, 13), 'updates': slice(13, 14),
    'coasted': slice(14, 15), 'breakdowns': slice(15, 16), 'z_min': slice(16, 17), 'z_max': slice(17, 18), 'd2_max': slice(18, 19),
    'd2_max_at': slice(19, 20), 'tilt_max': slice(20, 21), 'tilt_max_at': slice(21, 22), 'v2_max': slice(22, 23), 'w2_max': slice(23, 24),
    'first_fallen': slice(24, 25), 'last_out_of_band': slice(25, 26), 'in_band': slice(26, 27), 'torque_max': slice(27, 28),
    'torque_sq_sum': slice(28, 29), 'fz_max': slice(29, 30), 'stance_height_min': slice(30, 31), 'nan_records': slice(31, 32),
    'contact_switches': slice(32, 33), 'last_flags': slice(33, 37), 'contact_count': slice(37, 41), 'swing_height_max': slice(41, 42),
    'zero_42': slice(42, 43), 'torque_plant_records': slice(43, 44), 'clamped_records': slice(44, 45), 'clamped_joints_sum': slice(45, 46),
    'torque_deviation_max': slice(46, 47), 'stance_fz_min': slice(47, 48), 'pulling_records': slice(48, 49), 'accel_mismatch_max': slice(49, 50),
    'force_mismatch_max': slice(50, 51), 'ground_records': slice(51, 52), 'ground_contact_count': slice(52, 56), 'slip_sum': slice(56, 57),
    'plan_mismatch_sum': slice(57, 58), 'airborne_records': slice(58, 59), 'first_slip': slice(59, 60), 'ground_switches': slice(60, 61),
    'last_ground_contacts': slice(61, 62)}
STUDY_FIELDS = {
    'instances': slice(0, 1), 'fallen': slice(1, 2), 'settled': slice(2, 3), 'zero_action': slice(3, 4), 'settled_from_max': slice(4, 5),
    'settled_from_sum': slice(5, 6), 'd2_max': slice(6, 7), 'tilt_max': slice(7, 8), 'torque_max': slice(8, 9), 'qp_iters_sum': slice(9, 10),
    'clamped_records': slice(10, 11), 'pulling': slice(11, 12), 'slip_sum': slice(12, 13), 'plan_mismatch_sum': slice(13, 14),
    'breakdowns': slice(14, 15), 'stance_fz_min': slice(15, 16)}


def criteria(z_min, tilt_max, r2_settle, dz_settle, tilt_settle, v2_settle):
    """criteria[8]: fallen if p_z < z_min or u > tilt_max; in band if d2 <= r2_settle, |p_z - ref_z| <= dz_settle, u <= tilt_settle and
    |v_lin - v_ref|^2 <= v2_settle.  Squared quantities: d2 and v2 are squared norms, u = 2 (qx^2 + qy^2) = 1 - cos(tilt); the two reserved entries are 0"""
    return np.array([z_min, tilt_max, r2_settle, dz_settle, tilt_settle, v2_settle, 0.0, 0.0], dtype=np.float64)


def empty(instances):
    """summaries[instances][64] in the state after a reset (what the host fold starts from): counts and sums 0, maxima -inf, minima +inf, ordinals
    and carries -1"""
    s = np.zeros((int(instances), SUMMARY_DOUBLES))
    s[:, [6, 8, 12, 19, 21, 24, 25, 59, 33, 34, 35, 36, 61]] = -1.0
    s[:, [10, 17, 18, 20, 22, 23, 27, 29, 41, 46, 49, 50]] = -np.inf
    s[:, [16, 30, 47]] = np.inf
    return s


def _criteria_array(crit):
    a = np.ascontiguousarray(crit, dtype=np.float64)
    if a.shape != (CRITERIA_DOUBLES,):
        raise ValueError('criteria: %d doubles expected (criteria(...)), got shape %s' % (CRITERIA_DOUBLES, a.shape))
    return a


def _ref_array(ref, batch):
    r = np.asarray(ref, dtype=np.float64)
    if r.shape == (REF_DOUBLES,):
        r = np.tile(r, (batch, 1))
    if r.shape != (batch, REF_DOUBLES):
        raise ValueError('ref: shape (%d,) or (%d, %d) expected, got %s' % (REF_DOUBLES, batch, REF_DOUBLES, r.shape))
    return np.ascontiguousarray(r)


def reference_from_config(cfg, batch):
    """ref[batch][6]: the position of the configuration's tracking target (srb_target: p, h, quaternion, L) and its linear momentum over the mass"""
    t = np.asarray(cfg['srb_target'], dtype=np.float64)
    return np.tile(np.concatenate([t[:3], t[3:6] / float(cfg['mass'])]), (batch, 1))


def enable(mpc, crit, ref=None):
    """allocate and reset the tick summaries of the batch; crit: criteria(...); ref: [6] for the whole batch or [batch][6] = {p_ref, v_ref}, None:
    reference_from_config of the batch's configuration.  crit None: tick summaries off, buffers freed"""
    if crit is None:
        mpc._chk(mpc.L.srbm_tick_summary_enable(mpc.h, None, None))
        return
    r = _ref_array(reference_from_config(mpc.cfg, mpc.batch) if ref is None else ref, mpc.batch)
    mpc._chk(mpc.L.srbm_tick_summary_enable(mpc.h, _criteria_array(crit).ctypes.data_as(_dp), r.ctypes.data_as(_dp)))


def reset(mpc):
    """the summaries back to the state of empty(); asynchronous on the batch's stream"""
    mpc._chk(mpc.L.srbm_tick_summary_reset(mpc.h))


def _ticks_logged(mpc):
    n = C.c_int(0)
    mpc._chk(mpc.L.srbm_tick_log_count(mpc.h, C.byref(n)))
    return n.value


def fold(mpc, first_slot=0, count=None):
    """fold the tick-log slots [first_slot, first_slot + count) (None: up to the cursor) into the summaries; asynchronous on the batch's stream"""
    count = _ticks_logged(mpc) - first_slot if count is None else count
    mpc._chk(mpc.L.srbm_tick_summary_fold(mpc.h, int(first_slot), int(count)))


def fold_dev(mpc, log_ptr, slots, first_slot=0, count=None):
    """the same kernel on log[slots][batch][64] at device address log_ptr (any array of tick records; no tick log needed); asynchronous"""
    count = slots - first_slot if count is None else count
    mpc._chk(mpc.L.srbm_tick_summary_fold_dev(mpc.h, log_ptr, int(slots), int(first_slot), int(count)))


def summaries(mpc, first=0, count=None):
    """summaries[count][64] of instances [first, first + count); synchronous"""
    count = mpc.batch - first if count is None else count
    out = np.zeros((max(int(count), 0), SUMMARY_DOUBLES))
    mpc._chk(mpc.L.srbm_tick_summary_get(mpc.h, int(first), int(count), out.ctypes.data_as(_dp)))
    return out


def study(mpc):
    """the study record [16] of the batch's own summaries; synchronous"""
    out = np.zeros(STUDY_DOUBLES)
    mpc._chk(mpc.L.srbm_tick_study(mpc.h, out.ctypes.data_as(_dp)))
    return out


def study_dev(mpc, summaries_ptr, instances, study_ptr):
    """the study record of summaries[instances][64] at device address summaries_ptr (a gathered array) into device memory at study_ptr ([16]), on the
    batch's stream, no synchronisation"""
    mpc._chk(mpc.L.srbm_tick_study_dev(mpc.h, summaries_ptr, int(instances), study_ptr))


def allgather(mpc, comm, out_ptr):
    """this rank's summaries into their slot of out[world * batch][64] (device pointer) and ONE in-place ncclAllGather on the batch's stream; comm as
    BatchMPC.rccl_comm_init_rank returns it; asynchronous"""
    mpc._chk(mpc.L.srbm_tick_summary_allgather_dev(mpc.h, comm, out_ptr))


def settled(t):
    """bool[instances]: the instance did not fall and its last record is in band (field 24 < 0 and field 25 < field 0 - 1); settled from = field 25 + 1"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, SUMMARY_DOUBLES)
    return (t[:, 24] < 0) & (t[:, 25] < t[:, 0] - 1)


# ---- the same fold and reduction on the host (no GPU, no batch) ----
def fold_host(L, log, crit, ref, into=None, first_slot=0, count=None):
    """L: a loaded library (host.lib()); log[slots][batch][64]; ref[batch][6]; into: summaries[batch][64] to continue (None: empty()).
    Returns the summaries after folding the slots [first_slot, first_slot + count) in ascending order"""
    log = np.ascontiguousarray(log, dtype=np.float64)
    slots, batch = log.shape[0], log.shape[1]
    count = slots - first_slot if count is None else count
    out = empty(batch) if into is None else np.array(into, dtype=np.float64).reshape(batch, SUMMARY_DOUBLES)
    ref = _ref_array(ref, batch)
    rc = L.srbm_tick_fold_host(log.ctypes.data_as(_dp), slots, batch, int(first_slot), int(count), _criteria_array(crit).ctypes.data_as(_dp),
                               ref.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return out


def study_host(L, t):
    """the study record [16] of summaries[instances][64], instances in ascending order"""
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, SUMMARY_DOUBLES)
    out = np.zeros(STUDY_DOUBLES)
    if L.srbm_tick_study_host(t.ctypes.data_as(_dp), len(t), out.ctypes.data_as(_dp)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return out


# ---- the chunked driver ----
def _step_summaries_enabled(mpc):
    """whether rollout summaries (the step-log fold) are enabled on the batch, asked of the one entry that changes nothing and copies nothing: a get
    of zero instances, which is refused exactly when they are off"""
    return mpc.L.srbm_rollout_summary_get(mpc.h, 0, 0, np.zeros(1).ctypes.data_as(_dp)) == 0


def run(roll, ticks, chunk, ticks_per_update, tick_dt, first_tick=0, gait=None, gait_opt_freq=None):
    """ticks first_tick .. first_tick + ticks - 1 of controller_rollout.ControllerRollout `roll` in launches of `chunk` ticks: tick-log cursor to 0,
    roll.advance, the tick fold -- all queued on the batch's stream, ONE synchronisation at the end.  The tick log needs room for one chunk only
    (roll.tick_log_enable(chunk)); whatever it held before is overwritten.  If rollout summaries (rollout_summary.enable) are on as well, every chunk
    also folds the step log and sets its cursor to 0: the step log then needs room for the MPC updates of one chunk, and one run returns both levels
    of outcome"""
    if chunk < 1:
        raise ValueError('chunk: at least one tick')
    mpc = roll.mpc
    steps_too = _step_summaries_enabled(mpc)
    done = 0
    while done < ticks:
        n = min(chunk, ticks - done)
        roll.tick_log_reset()
        if steps_too:
            mpc.step_log_reset()
        roll.advance(first_tick + done, n, ticks_per_update, tick_dt, gait=gait, gait_opt_freq=gait_opt_freq)
        fold(mpc, 0, n)
        if steps_too:
            mpc._chk(mpc.L.srbm_rollout_summary_fold(mpc.h, 0, mpc.step_log_count()))
        done += n
    roll.tick_log_reset()
    if steps_too:
        mpc.step_log_reset()
    mpc.synchronize()
