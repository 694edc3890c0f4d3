"""The sensor model of whole-controller rollouts restated in Python from the tables of include/srbm_rti.h ("sensor model"), for
test_sensors_host.py and test_gpu_sensors.py: Philox4x32-10 on Python integers, the unit noise, and one tick of one instance in np.float64 scalars,
every rounded operation a statement of its own in the order the header writes it.  It is written per instance and per quantity (pose sample, ring
read, velocities, filter), not per measurement component as the library's function is, so the two are different programs.
A plain module: no fixtures, nothing pytest collects."""
import numpy as np

F = np.float64
M32 = 0xFFFFFFFF
SQRT3 = F(1.7320508075688772)
STATE_DOUBLES, RECORD_DOUBLES, RING = 72, 8, 5


def philox(counter, key):
    """Philox4x32-10: counter[4], key[2] of Python ints -> [4]"""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def unit_noise(seed, tick, channel):
    seed = int(seed)
    s = sum(philox((tick, channel, 0, 0), (seed & M32, seed >> 32)))
    d = F(s)
    assert int(d) == s
    u = d * F(2.0 ** -32)
    w = u - F(2.0)
    return w * SQRT3


def noisy(x, sigma, seed, tick, channel):
    if sigma == 0.0:
        return F(x)
    t = F(sigma) * unit_noise(seed, tick, channel)
    return F(x) + t


def state_init(q, v):
    """ms[72] of one instance at (q, v)"""
    ms = np.zeros(STATE_DOUBLES)
    for s in range(RING):
        ms[1 + 7 * s:8 + 7 * s] = q[:7]
    ms[36:54] = v
    ms[54:72] = v
    return ms


def pose_sample(S, seed, k, q):
    out = np.array(q[:7], F)
    for i in range(3):
        out[i] = noisy(q[i], S[2], seed, k, i)
    if S[3] != 0.0:
        a0, a1, a2, a3 = (F(x) for x in q[3:7])
        b0, b1, b2 = (F(0.5) * (F(S[3]) * unit_noise(seed, k, 3 + i)) for i in range(3))
        x = a3 * b0; x = x + a0; t = a1 * b2; x = x + t; t = a2 * b1; x = x - t
        y = a3 * b1; t = a0 * b2; y = y - t; y = y + a1; t = a2 * b0; y = y + t
        z = a3 * b2; t = a0 * b1; z = z + t; t = a1 * b0; z = z - t; z = z + a2
        w = a3; t = a0 * b0; w = w - t; t = a1 * b1; w = w - t; t = a2 * b2; w = w - t
        n2 = x * x; t = y * y; n2 = n2 + t; t = z * z; n2 = n2 + t; t = w * w; n2 = n2 + t
        a = F(3.0) - n2
        a = a * F(0.5)
        out[3:7] = [x * a, y * a, z * a, w * a]
    return out


def slot(n, behind):
    return (n - 1 - behind) % RING          # (Python's % is non-negative)


def rotation(qt):
    """Eigen's Quaterniond::matrix() for xyzw, every entry 1 - 2 (. + .) or 2 (. +- .) with each operation rounded"""
    x, y, z, w = (F(c) for c in qt)
    two, one = F(2.0), F(1.0)

    def diag(a, b):
        s = a * a + b * b          # (numpy scalars: the two products and the sum round separately)
        return one - two * s

    def off(a, b, c, d, sign):
        p, r = a * b, c * d
        return two * (p + r if sign > 0 else p - r)
    return np.array([[diag(y, z), off(x, y, z, w, -1), off(x, z, y, w, +1)],
                     [off(x, y, z, w, +1), diag(x, z), off(y, z, x, w, -1)],
                     [off(x, z, y, w, -1), off(y, z, x, w, +1), diag(x, y)]])


def measure_tick(S, seed, k, tick_dt, q, v, ms, srec):
    """one tick of one instance: sens S[16], the true (q, v); ms[72] and srec[8] are moved in place -> qm[19], vm[18]"""
    mt, delay = int(S[0]), int(S[1])
    n = int(ms[0])
    sample = k % mt == 0
    if sample:
        ms[1 + 7 * (n % RING):8 + 7 * (n % RING)] = pose_sample(S, seed, k, q)
        n += 1
        ms[0] = n
    qm, vm = np.zeros(19), np.zeros(18)
    avail = ms[1 + 7 * slot(n, delay):8 + 7 * slot(n, delay)].copy()
    prev = ms[1 + 7 * slot(n, delay + 1):8 + 7 * slot(n, delay + 1)].copy()
    qm[:7] = avail
    for j in range(12):
        qm[7 + j] = noisy(q[7 + j], S[10], seed, k, 12 + j)
    cur = np.zeros(18)
    if S[4] == 0.0:
        for i in range(3):
            cur[i] = noisy(v[i], S[5], seed, k, 6 + i)
    else:
        T = F(mt) * F(tick_dt)
        w = [(F(avail[i]) - F(prev[i])) / T for i in range(3)]
        R = rotation(avail[3:7])
        for i in range(3):
            m0, m1, m2 = R[0, i] * w[0], R[1, i] * w[1], R[2, i] * w[2]
            s = m0 + m1
            cur[i] = s + m2
    for i in range(3):
        x = F(v[3 + i])
        if S[7 + i] != 0.0:
            x = x + F(S[7 + i])
        cur[3 + i] = noisy(x, S[6], seed, k, 9 + i)
    for j in range(12):
        cur[6 + j] = noisy(v[6 + j], S[11], seed, k, 24 + j)
    for j in range(18):
        x = F(S[12] if j < 6 else S[13])
        out = F(cur[j])
        if x != 0.0:
            a = x / (F(1.0) + x)
            c = (F(1.0) - x) / (F(1.0) + x)
            s = F(cur[j]) + F(ms[36 + j])
            t1 = a * s
            t2 = c * F(ms[54 + j])
            out = t1 + t2
        ms[36 + j], ms[54 + j], vm[j] = cur[j], out, out
    srec[0] += 1
    srec[1] += 1 if sample else 0
    same_quat = np.array_equal(qm[3:7], np.asarray(q[3:7], float))
    dot = F(0.0)
    for i in range(4):
        t = F(qm[3 + i]) * F(q[3 + i])
        dot = t if i == 0 else dot + t
    errs = [np.abs(qm[:3] - q[:3]).max(), F(0.0) if same_quat else F(1.0) - dot * dot, np.abs(vm[:3] - v[:3]).max(), np.abs(vm[3:6] - v[3:6]).max(),
            np.abs(qm[7:] - q[7:]).max(), np.abs(vm[6:] - v[6:]).max()]
    for g, e in enumerate(errs):
        if e > srec[2 + g]:
            srec[2 + g] = e
    return qm, vm


def measure(first_tick, tick_dt, sens, seed, q_true, v_true, ms, srec=None):
    """the loop of srbm_sensor_measure_host: -> qm[ticks][batch][19], vm[ticks][batch][18], ms and srec after (the arguments are not modified)"""
    ticks, batch = q_true.shape[:2]
    ms = np.array(ms, float)
    srec = np.zeros((batch, RECORD_DOUBLES)) if srec is None else np.array(srec, float)
    qm, vm = np.zeros((ticks, batch, 19)), np.zeros((ticks, batch, 18))
    for k in range(ticks):
        for b in range(batch):
            qm[k, b], vm[k, b] = measure_tick(sens[b], int(seed[b]), first_tick + k, tick_dt, q_true[k, b], v_true[k, b], ms[b], srec[b])
    return qm, vm, ms, srec


def four_instances(tick_dt, record, lpf_x):
    """the four differing instances of the tests -> sens[4][16], seed[4]: mocap_ticks 1 / 2 / 3 / 5, delays 0..3, both velocity sources, filters on and off,
    instance 2 with a gyro bias only (record, lpf_x: srbm_loader.sensors')"""
    sens = np.array([
        record(mocap_ticks=1, mocap_delay=0, sigma_p=2e-3, sigma_r=5e-3, sigma_v=0.02, sigma_w=0.03, gyro_bias=(0.01, -0.02, 0.005), sigma_qj=1e-3, sigma_vj=0.05,
               lpf_base=lpf_x(15.0, tick_dt), lpf_joints=lpf_x(20.0, tick_dt)),
        record(mocap_ticks=2, mocap_delay=1, sigma_p=1e-3, sigma_r=2e-3, velocity_source=1, sigma_w=0.01, sigma_vj=0.02, lpf_joints=lpf_x(10.0, tick_dt)),
        record(mocap_ticks=3, mocap_delay=2, gyro_bias=(0.02, 0.0, -0.03)),
        record(mocap_ticks=5, mocap_delay=3, sigma_p=3e-3, velocity_source=1, sigma_qj=2e-3, lpf_base=lpf_x(8.0, tick_dt))])
    return sens, np.array([7 + 2 ** 32, 2 ** 63 + 11, 3, 0xDEADBEEFCAFEF00D], np.uint64)
