"""What the tests of the rollout's command schedule (test_commands_host.py, test_gpu_commands.py) share: the rule of include/srbm_rti.h ("timed
motion commands") restated in plain Python on np.float64 scalars, operation by operation and in the stated order -- the event in force, the target,
the anchor of a relative event, the two cost products with separately rounded products and sums, the state and the record --, the folding over a
sequence of updates, and the seeded inputs of the tests.  A plain module: no fixtures, nothing pytest collects."""
import numpy as np

f64 = np.float64
MAX_EVENTS, EVENT_DOUBLES, STATE_DOUBLES, REC_DOUBLES = 8, 28, 4, 32
T0, FLAGS, LEAD, RESERVED, DES, RATE = 0, 1, 2, 3, 4, 16


def event(t0, des12, rate12=None, lead=0.0, relative=False):
    e = np.zeros(EVENT_DOUBLES)
    e[T0], e[FLAGS], e[LEAD] = t0, 1.0 if relative else 0.0, lead
    e[DES:DES + 12] = des12
    if rate12 is not None:
        e[RATE:RATE + 12] = rate12
    return e


def initial(batch):
    cstate, crec = np.zeros((batch, STATE_DOUBLES)), np.zeros((batch, REC_DOUBLES))
    cstate[:, 0] = crec[:, 1] = -1.0
    return cstate, crec


def in_force(E, t):
    """E[n][28] of one instance -> the index of the last event with t0 <= t, -1: none"""
    e = -1
    for i in range(len(E)):
        if f64(E[i][T0]) <= f64(t):
            e = i
    return e


def cost_row(M, i, des):
    """-1 * sum_j M[12 i + j] des[j], j ascending, every product and every sum rounded on its own"""
    M = np.asarray(M, f64).reshape(144)
    a = f64(0.0)
    for j in range(12):
        p = f64(M[12 * i + j]) * f64(des[j])
        a = a + p
    return f64(-1.0) * a


def update(E, Q, Phi, t, state13, cstate, crec):
    """one MPC update of one instance at t on state13: -> (des[12], w[12], Phi_w[12]) or None where no event is in force; cstate[4] and crec[32] are
    folded into in place"""
    t = f64(t)
    idx = in_force(E, t)
    if idx < 0:
        return None
    ev = np.asarray(E[idx], f64)
    x, y = f64(state13[0]), f64(state13[1])
    latched = int(cstate[0]) == idx
    ax, ay = (f64(cstate[1]), f64(cstate[2])) if latched else (x, y)
    dt = t - ev[T0]
    s = dt + ev[LEAD]
    des = np.zeros(12)
    for i in range(12):
        p = ev[RATE + i] * s
        des[i] = ev[DES + i] + p
    unled = [ev[DES + i] + ev[RATE + i] * dt for i in range(2)]          # (two operations on f64 scalars: numpy does not fuse them)
    rel = ev[FLAGS] != 0.0
    if rel:
        des[0] = des[0] + ax
        des[1] = des[1] + ay
        unled[0] = unled[0] + ax
        unled[1] = unled[1] + ay
    w = np.array([cost_row(Q, i, des) for i in range(12)])
    pw = np.array([cost_row(Phi, i, des) for i in range(12)])
    if not latched:
        cstate[0], cstate[1], cstate[2], cstate[3] = idx, (ax if rel else 0.0), (ay if rel else 0.0), t
        crec[2] = crec[2] + 1.0
        crec[3], crec[4], crec[5] = t, cstate[1], cstate[2]
    crec[0] = crec[0] + 1.0
    crec[1] = idx
    dx, dy = x - unled[0], y - unled[1]
    dx2, dy2 = dx * dx, dy * dy
    d2 = dx2 + dy2
    d = np.sqrt(d2)
    if d > crec[6]:
        crec[6] = d
    crec[7] = crec[7] + d2
    crec[8:20] = des
    return des, w, pw


def fold(cmds, Q, Phi, times, states13, cstate=None, crec=None):
    """cmds[batch][n][28], Q / Phi[batch][144], times[n_updates][batch], states13[n_updates][batch][13] -> dict(des12, w12, Phi_w12 (NaN where no
    event is in force), cstate, crec) as srbm_command_target_host returns them"""
    batch = len(cmds)
    nu = len(times)
    cs0, cr0 = initial(batch)
    cs = cs0 if cstate is None else np.array(cstate, float)
    cr = cr0 if crec is None else np.array(crec, float)
    des, w, pw = (np.full((nu, batch, 12), np.nan) for _ in range(3))
    for u in range(nu):
        for b in range(batch):
            out = update(cmds[b], Q[b], Phi[b], times[u][b], states13[u][b], cs[b], cr[b])
            if out is not None:
                des[u, b], w[u, b], pw[u, b] = out
    return dict(des12=des, w12=w, Phi_w12=pw, cstate=cs, crec=cr)


# ---- the inputs of the tests ----
def cost_matrices(batch, seed=17):
    """per-instance weights -> Q[batch][144], Phi[batch][144]: diagonal with entries over four decades, Phi = 3 Q with other entries swapped in, and
    the LAST instance full, symmetric and positive definite in both"""
    rng = np.random.default_rng(seed)
    Q, Phi = np.zeros((batch, 12, 12)), np.zeros((batch, 12, 12))
    for b in range(batch):
        Q[b] = np.diag(10.0 ** rng.uniform(-1, 3, 12))
        Phi[b] = np.diag(3.0 * np.roll(np.diag(Q[b]), 1) + rng.uniform(0.1, 1.0, 12))
    for M, scale in ((Q, 1.0), (Phi, 2.5)):
        A = rng.normal(size=(12, 12))
        M[-1] = scale * (A @ A.T + 12 * np.eye(12))
    return Q.reshape(batch, 144), Phi.reshape(batch, 144)


def host_schedule(batch, times, seed=23):
    """the schedules of the host test on the update times `times` (ascending, at least 7), per instance three events with random targets and rates:
    event 0 absolute, beginning EXACTLY at times[1] (even instances) or strictly between times[0] and times[1] (odd ones); event 1 relative with a
    lead > 0, beginning strictly between times[2] and times[3] (in force at two updates); event 2 absolute again at times[5] -> cmds[batch][3][28].
    times[0] lies before every t0"""
    rng = np.random.default_rng(seed)
    cmds = np.zeros((batch, 3, EVENT_DOUBLES))
    for b in range(batch):
        t0 = times[1] if b % 2 == 0 else 0.5 * (times[0] + times[1]) + 1e-3 * rng.uniform()
        cmds[b, 0] = event(t0, rng.normal(size=12), rng.normal(size=12) * 0.3, lead=0.0 if b % 3 else 0.04)
        cmds[b, 1] = event(0.3 * times[2] + 0.7 * times[3],rng.normal(size=12) * 0.1, rng.normal(size=12) * 0.5, lead=0.02 + 0.01 * b, relative=True)
        cmds[b, 2] = event(times[5], rng.normal(size=12), rng.normal(size=12) * 0.2)
    return cmds


def host_states(n_updates, batch, seed=29):
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n_updates, batch, 13))
    s[:, :, 6:10] /= np.linalg.norm(s[:, :, 6:10], axis=2, keepdims=True)
    return s
