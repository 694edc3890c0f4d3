"""The synthetic workloads of SURVEY.md section 8(d) -- BASELINE.json's configurations B, C, D as seeded instance generators -- and the sharding of
a global batch over ranks (section 8e).  Used by bench.py, by the parity tests (the same seeded instances) and by the developer scripts."""
import numpy as np

# REFERENCE_SOLVER_SETTINGS -- (gap_abs, gap_rel, feas, max_iter) of srbm_set_solver_tolerances -- is defined once, in host.py beside the setter;
# srbm_loader hands it to this module under the same name (the two modules do not import each other)

# the nominal feet of the reference's simulation (test/simulation_mpc.cpp:104-108): FL FR RL RR
EE_NOMINAL = np.array([[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]], float)
EE_NOMINAL.setflags(write=False)           # one array for every caller


def shard_range(total, rank, world):
    """contiguous block [lo, hi) of `total` instances owned by `rank`"""
    per = total // world
    rem = total % world
    lo = rank * per + min(rank, rem)
    return lo, lo + per + (1 if rank < rem else 0)


def instances(cfg, make_inst, ids):
    """the seeded instances `ids` of a generator (config_b_instance, ...) as one batch: (states [B, 13], ees [B, 12]), contiguous float64.
    ids: an int B for range(B), or any iterable of instance numbers; cfg: one dict, or a list with one dict per instance (a heterogeneous batch)"""
    ids = list(range(ids)) if isinstance(ids, (int, np.integer)) else list(ids)
    cfgs = cfg if isinstance(cfg, (list, tuple)) else [cfg] * len(ids)
    if len(cfgs) != len(ids):
        raise ValueError('instances: %d configs for %d instances' % (len(cfgs), len(ids)))
    states, ees = zip(*[make_inst(c, b) for c, b in zip(cfgs, ids)])
    return np.ascontiguousarray(states, dtype=np.float64), np.ascontiguousarray(ees, dtype=np.float64).reshape(len(ids), 12)


def config_b_instance(cfg, b):
    """instance b of Config B: perturbed initial state + foot positions"""
    rng = np.random.Generator(np.random.MT19937(20240112 + b))
    u = lambda lo, hi: lo + (hi - lo) * rng.random()
    m = cfg['mass']
    p = np.array([u(-0.02, 0.02), u(-0.02, 0.02), 0.30 + u(-0.01, 0.01)])
    v = np.array([u(-0.5, 0.5), u(-0.5, 0.5), u(-0.1, 0.1)])
    rpy = np.array([u(-0.05, 0.05), u(-0.05, 0.05), u(-0.05, 0.05)])
    L = np.array([u(-0.1, 0.1), u(-0.1, 0.1), u(-0.1, 0.1)])
    th = np.linalg.norm(rpy)
    quat = np.concatenate([np.sin(th / 2) / th * rpy, [np.cos(th / 2)]])
    state = np.concatenate([p, m * v, quat, L])
    hips = np.array([[0.2055, 0.147], [0.2055, -0.147], [-0.1555, 0.147], [-0.1555, -0.147]])
    ee = np.zeros((4, 3))
    for e in range(4):
        ee[e, 0] = p[0] + hips[e, 0] + u(-0.02, 0.02)
        ee[e, 1] = p[1] + hips[e, 1] + u(-0.02, 0.02)
    return state, ee


def config_c_instance(cfg, b):
    """instance b of Config C: Config B's perturbations around the srb_init of apps/a1_gait_opt_config.yaml
    (height 0.34); the target of that file is x_des = y_des = 1"""
    state, ee = config_b_instance(cfg, b)
    state[2] += cfg['srb_init'][2] - 0.30
    return state, ee


def config_d_instance(cfg, b):
    """instance b of Config D: apps/a1_config_distr_rejection.yaml values (N=50, dt=0.02); the file's
    single push becomes a distribution -- lin-mom xy ~ N(0, 2.5^2) truncated at 3 sigma, yaw ang-mom ~ N(0, 0.2^2), seed 777 + b"""
    rng = np.random.Generator(np.random.MT19937(777 + b))
    def tnorm(sig):
        while True:
            v = rng.normal(0.0, sig)
            if abs(v) <= 3 * sig:
                return v
    state = np.array(cfg['srb_init'], float)
    state[3] += tnorm(2.5); state[4] += tnorm(2.5)
    state[12] += rng.normal(0.0, 0.2)
    return state, EE_NOMINAL.copy()


def heterogeneous_configs(base, q_diags, B, seed=4242, num_nodes=None):
    """B configs around `base` that differ in every per-instance field of the batch (srbm_batch_create_each, BatchMPC.from_configs): mass
    +-15 %, Ir scaled by 0.8 .. 1.2, friction 0.5 / 0.6, force bound 150 / 200, force cost 0 / 1e-3, a Q diagonal drawn from q_diags, a
    target with x, y in [0, 1] and height 0.28 .. 0.34.  The batch-wide fields (horizon, time step, foot geometry) are base's."""
    rng = np.random.Generator(np.random.MT19937(seed))
    cfgs = []
    for b in range(B):
        c = dict(base)
        if num_nodes is not None:
            c['num_nodes'] = num_nodes
        c['mass'] = base['mass'] * (1 + rng.uniform(-0.15, 0.15))
        c['Ir'] = (np.asarray(base['Ir'], float) * rng.uniform(0.8, 1.2)).tolist()
        c['friction_coef'] = (0.5, 0.6)[b % 2]
        c['force_bound'] = (150.0, 200.0)[(b // 2) % 2]
        c['force_cost'] = (0.0, 1e-3)[(b // 4) % 2]
        c['Q_srbd_diag'] = list(q_diags[int(rng.integers(len(q_diags)))])
        tgt = list(base['srb_target'])
        tgt[0], tgt[1], tgt[2] = rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.28, 0.34)
        c['srb_target'] = tgt
        cfgs.append(c)
    return cfgs
