"""The tick summaries restated (include/srbm_rti.h, "tick summaries"): a plain per-record Python loop written from the layout tables of the header,
every operation on Python floats (IEEE doubles, each one rounded), producing arrays whose BYTES the library's results are compared with
(gpu_kit.same_bytes).  A plain module like rollout_summary_kit.py: no fixtures, nothing pytest collects.

    empty_summary, fold_record, fold, study      the restatement
    synthetic_log, SYNTH_*                        the seeded 10-slot x 6-instance log of the host tests, events written in at known places
    criteria_of_log                               the four band criteria taken as medians over a log itself (the GPU tests)
"""
import math

import numpy as np

INF = float('inf')
ORDINALS_AND_CARRIES = (6, 8, 12, 19, 21, 24, 25, 59, 33, 34, 35, 36, 61)
MAXIMA = (10, 17, 18, 20, 22, 23, 27, 29, 41, 46, 49, 50)
MINIMA = (16, 30, 47)


def empty_summary():
    t = [0.0] * 64
    for i in ORDINALS_AND_CARRIES:
        t[i] = -1.0
    for i in MAXIMA:
        t[i] = -INF
    for i in MINIMA:
        t[i] = INF
    return t


def _bits(v):
    """a double read as a set of bits; a value that is none (negative, 2^53 or more, NaN) has no bit set"""
    if not (0.0 <= v < 2.0 ** 53):
        return 0
    return int(v)


def fold_record(T, R, crit, ref):
    """one tick record R[64] into the summary T (a list of 64 floats, changed in place)"""
    R = [float(v) for v in R]
    crit = [float(v) for v in crit]; ref = [float(v) for v in ref]
    k = T[0]
    T[0] = k + 1.0
    if k == 0.0:
        T[1] = R[0]; T[3] = R[1]
    T[2] = R[0]; T[4] = R[1]
    if R[2] != 0.0:                           # targets status
        T[5] += 1.0
        if T[6] < 0.0:
            T[6] = k
    if R[3] > 1.0:                            # QP status: a zero control action
        T[7] += 1.0
        if T[8] < 0.0:
            T[8] = k
    T[9] = T[9] + R[4]
    if R[4] > T[10]:
        T[10] = R[4]
    flags = _bits(R[5])
    if flags & 1:
        T[11] += 1.0; T[12] = k
    for bit, field in ((2, 13), (4, 14), (8, 15)):
        if flags & bit:
            T[field] += 1.0
    if any(math.isnan(v) for v in R[6:63]):
        T[31] += 1.0
        return
    first_valid = T[0] - 1.0 - T[31] == 0.0   # no record has set the carry of the desired contacts yet
    pz = R[8]
    if pz < T[16]:
        T[16] = pz
    if pz > T[17]:
        T[17] = pz
    dx = R[6] - ref[0]; dy = R[7] - ref[1]
    d2 = dx * dx + dy * dy                    # (Python rounds the two products and the sum one by one)
    if d2 > T[18]:
        T[18] = d2; T[19] = k
    u = 2.0 * (R[9] * R[9] + R[10] * R[10])
    if u > T[20]:
        T[20] = u; T[21] = k
    vx = R[13] - ref[3]; vy = R[14] - ref[4]; vz = R[15] - ref[5]
    v2 = (vx * vx + vy * vy) + vz * vz
    if v2 > T[22]:
        T[22] = v2
    w2 = (R[16] * R[16] + R[17] * R[17]) + R[18] * R[18]
    if w2 > T[23]:
        T[23] = w2
    if (pz < crit[0] or u > crit[1]) and T[24] < 0.0:
        T[24] = k
    if d2 <= crit[2] and abs(pz - ref[2]) <= crit[3] and u <= crit[4] and v2 <= crit[5]:
        T[26] += 1.0
    else:
        T[25] = k
    e = R[19] * R[19]
    if abs(R[19]) > T[27]:
        T[27] = abs(R[19])
    for j in range(1, 12):
        tau = R[19 + j]
        if abs(tau) > T[27]:
            T[27] = abs(tau)
        e = e + tau * tau
    T[28] = T[28] + e
    flags4 = R[43:47]
    for i in range(4):
        if R[33 + 3 * i] > T[29]:
            T[29] = R[33 + 3 * i]
        if flags4[i] == 1.0:
            if R[47 + i] < T[30]:
                T[30] = R[47 + i]
            T[37 + i] += 1.0
        if flags4[i] == 0.0 and R[47 + i] > T[41]:
            T[41] = R[47 + i]
    if not first_valid and flags4 != T[33:37]:
        T[32] += 1.0
    T[33:37] = flags4
    if R[57] == 1.0:
        T[43] += 1.0
        if R[58] > 0.0:
            T[44] += 1.0
        T[45] = T[45] + R[58]
        if R[59] > T[46]:
            T[46] = R[59]
        if R[60] < T[47]:
            T[47] = R[60]
        if R[60] < 0.0:
            T[48] += 1.0
        if R[61] > T[49]:
            T[49] = R[61]
        if R[62] > T[50]:
            T[50] = R[62]
    if 4096.0 <= R[63] < 8192.0:
        word = _bits(R[63] - 4096.0)
        first_ground = T[51] == 0.0
        T[51] += 1.0
        for i in range(4):
            if word >> i & 1:
                T[52 + i] += 1.0
        slips = float(bin(word >> 4 & 15).count('1'))
        T[56] = T[56] + slips
        T[57] = T[57] + float(bin(word >> 8 & 15).count('1'))
        contact = float(word & 15)
        if contact == 0.0:
            T[58] += 1.0
        if slips > 0.0 and T[59] < 0.0:
            T[59] = k
        if not first_ground and contact != T[61]:
            T[60] += 1.0
        T[61] = contact


def fold(log, crit, ref, into=None, first=0, count=None):
    """log[slots][batch][64] -> summaries[batch][64] (float64 array); into: summaries to continue"""
    log = np.asarray(log, dtype=np.float64)
    slots, batch = log.shape[:2]
    count = slots - first if count is None else count
    out = np.zeros((batch, 64))
    for b in range(batch):
        T = empty_summary() if into is None else [float(v) for v in into[b]]
        for s in range(first, first + count):
            fold_record(T, log[s, b], crit, ref[b])
        out[b] = T
    return out


def study(summaries):
    U = [0.0] * 16
    U[4] = -1.0; U[6] = -INF; U[7] = -INF; U[8] = -INF; U[15] = INF
    for T in np.asarray(summaries, dtype=np.float64).reshape(-1, 64):
        T = [float(v) for v in T]
        U[0] += 1.0
        if T[24] >= 0.0:
            U[1] += 1.0
        if T[24] < 0.0 and T[25] < T[0] - 1.0:
            sf = T[25] + 1.0
            U[2] += 1.0
            if sf > U[4]:
                U[4] = sf
            U[5] = U[5] + sf
        if T[7] > 0.0:
            U[3] += 1.0
        if T[18] > U[6]:
            U[6] = T[18]
        if T[20] > U[7]:
            U[7] = T[20]
        if T[27] > U[8]:
            U[8] = T[27]
        U[9] = U[9] + T[9]
        U[10] = U[10] + T[44]
        if T[48] > 0.0:
            U[11] += 1.0
        U[12] = U[12] + T[56]
        U[13] = U[13] + T[57]
        U[14] = U[14] + T[15]
        if T[47] < U[15]:
            U[15] = T[47]
    return np.array(U)


# ---- the synthetic tick log of the host tests: batch 6 x 10 slots ----
SYNTH_SLOTS, SYNTH_BATCH = 10, 6
SYNTH_CRIT = np.array([0.15, 0.5, 0.0025, 0.05, 0.1, 1.0, 0.0, 0.0])
SYNTH_REF = np.array([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0]] * SYNTH_BATCH) + np.arange(SYNTH_BATCH)[:, None] * np.array([0.01, -0.01, 0.0, 0.1, 0.0, 0.0])
GROUND_WORDS = [15, 15, 15 | 32, 15 | 32 | 64, 15, 0xF00, 11 | 1024, 11, 11 | 16, 11]          # instance 3, by slot


def synthetic_log():
    """Random records (seeded) that are in band, with targets and QP solved, in full desired contact and of plant kind 0 unless an event says
    otherwise.  The events, by instance:
      0  kind 0.  Falls by height at slot 3; targets status 1 at slot 2 and 2 at slot 5; QP status 8 with the coast flag at slot 6; pushed at slots
         1 and 4, an update after slots 4 and 9; a field 5 that holds no set of bits at slots 7 (-3) and 8 (2^53)
      1  kind 1 without a ground.  Falls by tilt at slot 6; a NaN torque at slot 4, on a record that carries flag bit 3 (counted) and a negative
         field 60 (not counted); clamped joints at slots 2 and 7; a negative field 60 at slots 3 and 8; foot 3 never in desired contact
      2  kind 0.  Equal maxima of d2 at slots 2 and 7 and of u at slots 1 and 5 (the first must keep the ordinal); desired-contact switches at slots
         3 and 6; in band again from slot 8 on
      3  kind 1 on a ground, words GROUND_WORDS: slip bits at slots 2, 3 (two) and 8, mismatch bits at slots 5 (four) and 6, airborne at slot 5,
         ground contacts 15 -> 0 -> 11; one clamped joint at slot 3
      4  kind 0.  Out of band by height until slot 5, in band from slot 6 on: ends in band; a NaN in field 5 at slot 1
      5  kind 0.  In band throughout but for its last record, which leaves the band by velocity; a field 63 that is no ground word at slots 2..7
         (-4096, NaN, 2^53, 8192, 4095, 1e300)"""
    rng = np.random.default_rng(31)
    log = np.zeros((SYNTH_SLOTS, SYNTH_BATCH, 64))
    for s in range(SYNTH_SLOTS):
        for b in range(SYNTH_BATCH):
            r = log[s, b]
            r[0] = 100 + s; r[1] = 0.001 * (100 + s); r[4] = float(rng.integers(3, 13))
            r[6:9] = SYNTH_REF[b, :3] + rng.uniform(-0.01, 0.01, 3)
            q = np.concatenate([rng.uniform(-0.05, 0.05, 3), [1.0]])
            r[9:13] = q / np.linalg.norm(q)
            r[13:16] = SYNTH_REF[b, 3:] + rng.uniform(-0.05, 0.05, 3)
            r[16:19] = rng.uniform(-0.2, 0.2, 3)
            r[19:31] = rng.uniform(-10.0, 10.0, 12)
            for e in range(4):
                r[31 + 3 * e:34 + 3 * e] = [rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(20, 60)]
            r[43:47] = 1.0
            r[47:51] = rng.uniform(0.0, 0.002, 4)
            r[51:57] = rng.uniform(-1.0, 1.0, 6)
    I0, I1, I2, I3, I4, I5 = range(6)
    log[3, I0, 8] = 0.1                                             # fall by height
    log[2, I0, 2] = 1.0; log[5, I0, 2] = 2.0
    log[6, I0, 3] = 8.0; log[6, I0, 5] = 4.0                       # a zero control action: the kind-0 plant coasts
    log[1, I0, 5] = 1.0; log[4, I0, 5] = 3.0; log[9, I0, 5] = 2.0
    log[7, I0, 5] = -3.0; log[8, I0, 5] = 2.0 ** 53
    for b in (I1, I3):                                              # the torque-driven plant's fields
        log[:, b, 57] = 1.0
        log[:, b, 59] = rng.uniform(0.0, 1.0, SYNTH_SLOTS); log[:, b, 60] = rng.uniform(5.0, 20.0, SYNTH_SLOTS)
        log[:, b, 61] = rng.uniform(0.0, 3.0, SYNTH_SLOTS); log[:, b, 62] = rng.uniform(0.0, 9.0, SYNTH_SLOTS)
    log[6, I1, 9:13] = [0.6, 0.0, 0.0, 0.8]                         # u = 0.72 > 0.5: fall by tilt
    log[4, I1, 25] = np.nan; log[4, I1, 5] = 8.0; log[4, I1, 60] = -7.0
    log[2, I1, 58] = 2.0; log[7, I1, 58] = 3.0
    log[3, I1, 60] = -1.5; log[8, I1, 60] = -0.25
    log[:, I1, 46] = 0.0; log[:, I1, 50] = 0.05 + 0.003 * np.arange(SYNTH_SLOTS); log[:, I1, 40:43] = 0.0
    log[[2, 7], I2, 6] = SYNTH_REF[I2, 0] + 0.125; log[[2, 7], I2, 7] = SYNTH_REF[I2, 1]
    log[[1, 5], I2, 9:13] = [0.25, 0.0, 0.0, 0.96824583655185422]
    log[3:, I2, 43] = 0.0; log[6:, I2, 44] = 0.0                    # desired-contact switches at slots 3 and 6
    log[:, I3, 63] = 4096.0 + np.array(GROUND_WORDS, float)
    log[3, I3, 58] = 1.0
    log[:6, I4, 8] = SYNTH_REF[I4, 2] + 0.08                        # out of band by height until slot 5
    log[1, I4, 5] = np.nan
    log[9, I5, 13] = SYNTH_REF[I5, 3] + 3.0                         # |v - v_ref|^2 > 8 on the last record
    log[2:8, I5, 63] = [-4096.0, np.nan, 2.0 ** 53, 8192.0, 4095.0, 1e300]
    return log


def criteria_of_log(log, ref):
    """(r2_settle, dz_settle, tilt_settle, v2_settle): the medians of d2, |p_z - ref_z|, u and |v - v_ref|^2 over all records of
    log[slots][batch][64] -- criteria taken from the log itself, so that both outcomes of each band condition occur"""
    d = log[:, :, 6:8] - ref[None, :, 0:2]
    v = log[:, :, 13:16] - ref[None, :, 3:6]
    u = 2.0 * (log[:, :, 9] ** 2 + log[:, :, 10] ** 2)
    return (float(np.median((d ** 2).sum(-1))), float(np.median(np.abs(log[:, :, 8] - ref[None, :, 2]))), float(np.median(u)),
            float(np.median((v ** 2).sum(-1))))
