"""The rollout summaries restated (include/srbm_rti.h, "rollout summaries"): a plain per-record Python loop written from the layout tables of the header,
every operation on Python floats (IEEE doubles, each one rounded), producing arrays whose BYTES the library's results are compared with
(gpu_kit.same_bytes).  A plain module like gpu_kit.py: no fixtures, nothing pytest collects.

    empty_summary, fold_record, fold, study      the restatement
    synthetic_log, SYNTH_*                        the seeded 9-slot x 5-instance log of the host tests, events written in at known places
    medians_of_log                                settle radius and momentum band taken from a log itself (the GPU tests)
"""
import math

import numpy as np

INF = float('inf')
ORDINALS = (6, 18, 20, 23, 24)
MAXIMA = (10, 12, 14, 16, 17, 19, 21, 22, 26)
MINIMA = (13, 15, 27)


def empty_summary():
    s = [0.0] * 64
    for i in ORDINALS:
        s[i] = -1.0
    for i in MAXIMA:
        s[i] = -INF
    for i in MINIMA:
        s[i] = INF
    return s


def _or(a, b):
    if not (0.0 <= b < 2.0 ** 53):            # no set of bits: adds nothing
        return a
    return float(int(a) | int(b))


def fold_record(S, R, crit, ref, mu):
    """one record R[64] into the summary S (a list of 64 floats, changed in place)"""
    R = [float(v) for v in R]
    crit = [float(v) for v in crit]; ref = [float(v) for v in ref]; mu = float(mu)
    k = S[0]
    S[0] = k + 1.0
    if k == 0.0:
        S[1] = R[0]; S[3] = R[1]
    S[2] = R[0]; S[4] = R[1]
    if R[2] != 0.0:                           # status != Solved
        S[5] += 1.0
        if S[6] < 0.0:
            S[6] = k
    if R[2] > 1.0:                            # status > SolvedInacc
        S[7] += 1.0
    S[8] = _or(S[8], R[3])
    S[9] = S[9] + R[11]
    if R[11] > S[10]:
        S[10] = R[11]
    S[11] = S[11] + R[8]
    if R[9] > S[12]:
        S[12] = R[9]
    if R[7] < S[13]:
        S[13] = R[7]
    if R[10] > S[14]:
        S[14] = R[10]
    if R[58] == 1.0:
        S[38] += 1.0
        S[40] = S[40] + R[61]
    if R[58] == 2.0:
        S[39] += 1.0
        if R[62] > 0.0:
            S[41] += 1.0
        S[42] = R[63]
    if any(math.isnan(v) for v in R[17:30] + R[42:58]):
        S[28] += 1.0
        return
    first_valid = S[0] - 1.0 - S[28] == 0.0   # no record has set the carry yet
    pz = R[19]
    if pz < S[15]:
        S[15] = pz
    if pz > S[16]:
        S[16] = pz
    dx = R[17] - ref[0]; dy = R[18] - ref[1]
    d2 = dx * dx + dy * dy                    # (Python rounds the two products and the sum one by one)
    if d2 > S[17]:
        S[17] = d2; S[18] = k
    u = 2.0 * (R[23] * R[23] + R[24] * R[24])
    if u > S[19]:
        S[19] = u; S[20] = k
    hx = R[20] - ref[3]; hy = R[21] - ref[4]; hz = R[22] - ref[5]
    h2 = (hx * hx + hy * hy) + hz * hz
    if h2 > S[21]:
        S[21] = h2
    l2 = (R[27] * R[27] + R[28] * R[28]) + R[29] * R[29]
    if l2 > S[22]:
        S[22] = l2
    if (pz < crit[0] or u > crit[1]) and S[23] < 0.0:
        S[23] = k
    if d2 <= crit[2] and abs(pz - ref[2]) <= crit[3] and u <= crit[4] and h2 <= crit[5]:
        S[25] += 1.0
    else:
        S[24] = k
    flags = R[54:58]
    for e in range(4):
        fx, fy, fz = R[42 + 3 * e:45 + 3 * e]
        if fz > S[26]:
            S[26] = fz
        if flags[e] == 1.0:
            margin = mu * fz - max(abs(fx), abs(fy))
            if margin < S[27]:
                S[27] = margin
            S[34 + e] += 1.0
    if not first_valid and flags != S[30:34]:
        S[29] += 1.0
    S[30:34] = flags


def fold(log, crit, ref, mu, into=None, first=0, count=None):
    """log[slots][batch][64] -> summaries[batch][64] (float64 array); into: summaries to continue"""
    log = np.asarray(log, dtype=np.float64)
    slots, batch = log.shape[:2]
    count = slots - first if count is None else count
    out = np.zeros((batch, 64))
    for b in range(batch):
        S = empty_summary() if into is None else [float(v) for v in into[b]]
        for s in range(first, first + count):
            fold_record(S, log[s, b], crit, ref[b], mu[b])
        out[b] = S
    return out


def study(summaries):
    T = [0.0] * 16
    T[4] = -1.0; T[6] = -INF; T[7] = -INF; T[8] = INF
    for S in np.asarray(summaries, dtype=np.float64).reshape(-1, 64):
        S = [float(v) for v in S]
        T[0] += 1.0
        if S[23] >= 0.0:
            T[1] += 1.0
        if S[23] < 0.0 and S[24] < S[0] - 1.0:
            sf = S[24] + 1.0
            T[2] += 1.0
            if sf > T[4]:
                T[4] = sf
            T[5] = T[5] + sf
        if S[7] > 0.0:
            T[3] += 1.0
        if S[17] > T[6]:
            T[6] = S[17]
        if S[19] > T[7]:
            T[7] = S[19]
        if S[27] < T[8]:
            T[8] = S[27]
        T[9] = T[9] + S[9]
        T[10] = _or(T[10], S[8])
    return np.array(T)


# ---- the synthetic log of the host tests: batch 5 x 9 slots ----
SYNTH_SLOTS, SYNTH_BATCH = 9, 5
SYNTH_CRIT = np.array([0.15, 0.5, 0.04, 0.05, 0.1, 4.0, 0.0, 0.0])
SYNTH_REF = np.array([[0.0, 0.0, 0.3, 0.0, 0.0, 0.0]] * SYNTH_BATCH) + np.arange(SYNTH_BATCH)[:, None] * np.array([0.01, -0.01, 0.0, 0.1, 0.0, 0.0])
SYNTH_MU = np.array([0.5, 0.6, 0.7, 0.4, 0.55])


def synthetic_log():
    """Random records (seeded) that are in band, solved and in full contact unless an event says otherwise.  The events, by (slot, instance):
      instance 0: falls by height at slot 3; status 1 at slot 2, status 3 at slot 5; error bits 128 at slot 1 and 2 at slot 6
      instance 1: falls by tilt at slot 6; NaN forces and flag -1 of foot 2 at slot 4; foot 3 never in contact
      instance 2: equal maxima of d2 at slots 2 and 7 and of u at slots 1 and 5 (the first must keep the ordinal); contact switches at slots 3 and 6
      instance 3: gait kind 1 at slots 3 and 8 (pred_red 0.25 and 0.5), kind 2 at slots 4 and 5 (imin 0 and 3); out of band by height until
                  slot 5, in band from slot 6 on: ends in band
      instance 4: in band throughout but for its last record (slot 8), which leaves the band by momentum"""
    rng = np.random.default_rng(20)
    log = np.zeros((SYNTH_SLOTS, SYNTH_BATCH, 64))
    for s in range(SYNTH_SLOTS):
        for b in range(SYNTH_BATCH):
            r = log[s, b]
            r[0] = 10 + s + 1; r[1] = 0.05 * (s + 1); r[5] = 300; r[6] = 700
            r[7] = rng.uniform(0.5, 1.0); r[8] = rng.uniform(1.0, 9.0); r[9] = rng.uniform(0, 1e-3); r[10] = rng.uniform(0, 2.0)
            r[11] = float(rng.integers(8, 25)); r[12:15] = rng.uniform(0, 1e-9, 3); r[15] = -rng.uniform(1, 2); r[16] = -rng.uniform(0, 1)
            r[17:20] = SYNTH_REF[b, :3] + rng.uniform(-0.02, 0.02, 3)
            r[20:23] = SYNTH_REF[b, 3:] + rng.uniform(-0.5, 0.5, 3)
            q = np.concatenate([rng.uniform(-0.05, 0.05, 3), [1.0]])
            r[23:27] = q / np.linalg.norm(q)
            r[27:30] = rng.uniform(-0.2, 0.2, 3)
            r[30:42] = rng.uniform(-0.2, 0.2, 12)
            for e in range(4):
                r[42 + 3 * e:45 + 3 * e] = [rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(20, 60)]
            r[54:58] = 1.0
    I0, I1, I2, I3, I4 = range(5)
    log[3, I0, 19] = 0.1                                            # fall by height
    log[2, I0, 2] = 1.0; log[5, I0, 2] = 3.0
    log[1, I0, 3] = 128.0; log[6, I0, 3] = 2.0
    q = np.array([0.6, 0.0, 0.0, 0.8]); log[6, I1, 23:27] = q      # u = 0.72 > 0.5: fall by tilt
    log[4, I1, 48:51] = np.nan; log[4, I1, 56] = -1.0              # foot 2: spline lookup failed
    log[:, I1, 57] = 0.0; log[:, I1, 51:54] = [0.0, 0.0, -50.0]    # foot 3 never in contact (its force row would give a negative margin)
    log[[2, 7], I2, 17] = SYNTH_REF[I2, 0] + 0.125; log[[2, 7], I2, 18] = SYNTH_REF[I2, 1]
    log[[1, 5], I2, 23:27] = [0.25, 0.0, 0.0, 0.96824583655185422]
    log[3:, I2, 54] = 0.0; log[6:, I2, 55] = 0.0                   # switches at slots 3 and 6
    log[3, I3, 58] = 1.0; log[3, I3, 61] = 0.25; log[8, I3, 58] = 1.0; log[8, I3, 61] = 0.5
    log[4, I3, 58] = 2.0; log[4, I3, 62] = 0.0; log[4, I3, 63] = 0.011
    log[5, I3, 58] = 2.0; log[5, I3, 62] = 3.0; log[5, I3, 63] = 0.0075
    log[:6, I3, 19] = SYNTH_REF[I3, 2] + 0.08                       # out of band by height until slot 5
    log[8, I4, 20] = SYNTH_REF[I4, 3] + 3.0                         # |h - h_ref|^2 >= 9 - ... > 4 on the last record
    return log


def medians_of_log(log, ref):
    """(median of d2, median of |h - h_ref|^2) over all records of log[slots][batch][64]: criteria taken from the log itself"""
    d = log[:, :, 17:19] - ref[None, :, 0:2]
    h = log[:, :, 20:23] - ref[None, :, 3:6]
    return float(np.median((d ** 2).sum(-1))), float(np.median((h ** 2).sum(-1)))
