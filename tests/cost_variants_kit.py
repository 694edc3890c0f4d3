"""Cost sets whose final cost is NOT the tracking cost (a plain module: nothing pytest collects).

Every constructor of the project and of the oracle sets Phi = Q and Phi_w = -Q des = w (mpc_controller.cpp:57-67), so the lines that choose between
the two costs -- node N of the condensing, of the costates, of the merit and of the sensitivity right-hand side -- would go unobserved.  The four
sets below give them different data, over both the diagonal and the full 12 x 12 path of the kernels (q_diag of csrc/srbm_capi.hip):

    set  Q          Phi         Phi_w        path
    A    diag(q)    diag(10 q)  -Phi des2    diagonal path, final cost its own
    B    spd(99)    spd(7, 4)   -Phi des2    full path, both matrices
    C    diag(q)    spd(7, 4)   -Phi des2    q_diag cleared by Phi alone
    D    spd(99)    0           0            only the 1e-3 regularisation on the last node

q: the config's Q_srbd_diag; des: the tangent of its srb_target; des2: des shifted by (+0.3, -0.2, +0.03) in position.  All matrices are symmetric
(to rounding); the seeds are fixed.  Used on the device through the _each setters and on the oracle through OracleMPC.set_costs."""
import numpy as np

from srbm_loader import host

SETS = ('A', 'B', 'C', 'D')
DES2_SHIFT = (0.3, -0.2, 0.03)


def spd(cfg, seed, scale=1.0):
    """a full symmetric positive-definite matrix around scale x the config's diagonal: diag(sqrt(scale q)) (I + R R') diag(sqrt(scale q)), R uniform
    in +-0.2"""
    rng = np.random.Generator(np.random.MT19937(seed))
    d = np.sqrt(scale * np.asarray(cfg['Q_srbd_diag'], float))
    R = rng.uniform(-0.2, 0.2, (12, 12))
    return np.diag(d) @ (np.eye(12) + R @ R.T) @ np.diag(d)


def targets(cfg):
    """(des, des2)"""
    des = host.manifold_to_tangent(cfg['srb_target'])
    des2 = des.copy()
    des2[:3] += DES2_SHIFT
    return des, des2


def cost_set(cfg, name):
    """(des, Q, Phi, Phi_w) of set `name`"""
    q = np.asarray(cfg['Q_srbd_diag'], float)
    des, des2 = targets(cfg)
    Q = {'A': np.diag(q), 'B': spd(cfg, 99), 'C': np.diag(q), 'D': spd(cfg, 99)}[name]
    Phi = {'A': np.diag(10 * q), 'B': spd(cfg, 7, 4), 'C': spd(cfg, 7, 4), 'D': np.zeros((12, 12))}[name]
    return des, Q, Phi, -1 * Phi @ des2


def tracking_as_final(costs):
    """the same set with Phi, Phi_w := Q, w: what a kernel that never looked at the final cost would solve"""
    des, Q, _, _ = costs
    return des, Q, Q, -1 * Q @ des


def plain_costs(cfg):
    """what every constructor sets (host.BatchMPC.__init__, orc_mpc_create): (des, diag q, diag q, -diag(q) des)"""
    Q = np.diag(np.asarray(cfg['Q_srbd_diag'], float))
    des = host.manifold_to_tangent(cfg['srb_target'])
    return des, Q, Q, -1 * Q @ des


def expected_cost_blocks(cfg, costs):
    """(P, q) of the state part of the QP as the reference assembles it (mpc.cpp:542-564, :1090-1095): Q + 1e-3 I and w on nodes 0 .. N-1,
    Phi + 1e-3 I and Phi_w on node N"""
    N = int(cfg['num_nodes'])
    des, Q, Phi, Phi_w = costs
    nx = 12 * (N + 1)
    P = np.zeros((nx, nx)); q = np.zeros(nx)
    w = np.zeros(12)
    for i in range(12):                  # term by term in the order of mpc.cpp:137-151 (a BLAS product may add in another order)
        a = 0.0
        for j in range(12):
            a += Q[i, j] * des[j]
        w[i] = -1 * a
    for k in range(N + 1):
        s = slice(12 * k, 12 * k + 12)
        P[s, s] = (Phi if k == N else Q) + 1e-3 * np.eye(12)
        q[s] = Phi_w if k == N else w
    return P, q


def install(g, first, costs_each):
    """the three per-instance setters of the device batch g for instances first, first + 1, ..."""
    des, Q, Phi, Phi_w = (np.stack([c[k] for c in costs_each]) for k in range(4))
    g.add_quadratic_tracking_cost_each(first, des, Q)
    g.set_quadratic_final_cost_each(first, Phi)
    g.set_linear_final_cost_each(first, Phi_w)
