"""ctypes wrapper over oracle/liboracle.so (the CPU restatement of the reference; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from srbm_loader.host import C_TYPES, declare, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, 'oracle')
CONFIG_DIR = os.path.join(ROOT, 'bilevel-gait-gen_amd', 'configs')

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


class OrcConfig(C.Structure):
    _fields_ = [('num_nodes', C.c_int), ('dt', C.c_double), ('friction_coef', C.c_double), ('force_bound', C.c_double),
                ('swing_height', C.c_double), ('foot_offset', C.c_double), ('box_x', C.c_double), ('box_y', C.c_double),
                ('force_cost', C.c_double), ('mass', C.c_double), ('Ir', C.c_double * 9), ('hip_xy', C.c_double * 8),
                ('Q_diag', C.c_double * 12), ('des_state', C.c_double * 13)]


# every function of oracle/oracle_capi.cpp in the spelling of host.PROTOTYPES (handles are void*); tests/test_abi_prototypes.py holds the table to
# that file and to the symbols of liboracle.so
PROTOTYPES = prototypes('''\
void* orc_mpc_create(orc_config*)
void orc_mpc_destroy(void*)
void* orc_mpc_clone(void*)
char* orc_mpc_error(void*)
void orc_mpc_set_costs(void*, double*, double*, double*, double*)
void orc_mpc_set_warmstart(void*, double*)
int orc_mpc_initial_run(void*, double*, double*)
int orc_mpc_solve(void*, double*, double, double*)
int orc_mpc_rti(void*, double*, double, double*)
void orc_mpc_set_max_iter(void*, int)
void orc_mpc_sizes(void*, int*)
void orc_mpc_get_x(void*, double*)
void orc_mpc_get_qp_x(void*, double*)
void orc_mpc_get_z(void*, double*)
void orc_mpc_get_s(void*, double*)
void orc_mpc_get_states(void*, double*)
void orc_mpc_get_stats(void*, double*)
void orc_mpc_get_qp_dense(void*, double*, double*, double*, double*)
int orc_mpc_constraint_nnz(void*)
int orc_mpc_get_knots(void*, int, double*, int*, int*, double*, int*, double*)
double orc_mpc_init_time(void*)
int orc_mpc_get_contact_times(void*, int, double*, int*)
int orc_mpc_set_contact_times(void*, int, int*, double*)
int orc_mpc_adjust_for_current_contacts(void*, double, int*)
double orc_mpc_ee_value(void*, int, int, int, double)
int orc_mpc_plant_integrate(void*, double*, double, double, int, int, double*)
int orc_gait_gradient(void*, double*)
int orc_gait_get_d(void*, double*)
int orc_gait_param_partials(void*, void*, int, int, double*, double*, double*, double*)
int orc_gait_optimize(void*, double, double*, double*)
int orc_gait_line_search(void*, double*, double, double*, double*)
int orc_gait_line_search_q(void*, double*, double, double*, double*, int*)
int orc_qp_solve(int, int, int, int*, int*, double*, double*, int, int*, int*, double*, double*, int, int*, int*, double, double, double*, double*, double*, int*)
void orc_qp_sensitivity(int, int, int, double*, double*, double*, double*, double*, double*, double*, double*, double*, double*, double*)
void* orc_spline_create(int, double*, int, int)
void* orc_spline_clone(void*)
void orc_spline_destroy(void*)
double orc_spline_value_at(void*, int, int, double)
int orc_spline_lin(void*, int, int, double, double*)
int orc_spline_vars_idx(void*, int, int, double, int*)
int orc_spline_is_force_mutable(void*, double)
void orc_spline_add_poly(void*, double)
int orc_spline_remove_poly(void*, double)
int orc_spline_set_vars(void*, int, int, int, double, double)
int orc_spline_mutable_nodes(void*, int, int, int*)
int orc_spline_times(void*, double*, int*)
int orc_spline_node_type(void*, int, int, int)
int orc_spline_qp_vec(void*, int, int, double*)
double orc_spline_end_time(void*)
double orc_spline_start_time(void*)
int orc_spline_contact_times(void*, double*)
int orc_spline_set_contact_times(void*, int, double*)
double orc_spline_partial_wrt_time(void*, int, int, double, int)
int orc_spline_coef_partial_wrt_time(void*, int, int, double, int, double, double*)
void orc_quat_exp3(double*, double*)
void orc_quat_log3(double*, double*)''', dict(C_TYPES, **{'orc_config*': C.POINTER(OrcConfig)}))


def load_config(name='a1_configuration', **overrides):
    cfg = json.load(open(os.path.join(CONFIG_DIR, name + '.json')))
    cfg.update(overrides)
    return cfg


def build_oracle():
    subprocess.check_call(['make', '-s', '-C', ORACLE_DIR])
    return os.path.join(ORACLE_DIR, 'liboracle.so')


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ORACLE_DIR, 'liboracle.so')
        if not os.path.exists(path):
            build_oracle()
        _lib = declare(C.CDLL(path), PROTOTYPES)
    return _lib


def make_c_config(cfg):
    c = OrcConfig()
    c.num_nodes = int(cfg['num_nodes'])
    c.dt = cfg['integrator_dt']
    c.friction_coef = cfg['friction_coef']
    c.force_bound = cfg['force_bound']
    c.swing_height = cfg['swing_height']
    c.foot_offset = cfg['foot_offset']
    c.box_x, c.box_y = cfg['ee_box_size']
    c.force_cost = cfg['force_cost']
    c.mass = cfg['mass']
    c.Ir[:] = list(np.asarray(cfg['Ir'], float).reshape(-1))
    c.hip_xy[:] = list(np.asarray(cfg['hip_xy'], float).reshape(-1))
    c.Q_diag[:] = [float(v) for v in cfg['Q_srbd_diag']]
    c.des_state[:] = [float(v) for v in cfg['srb_target']]
    return c


class OracleMPC:
    """One MPCSingleRigidBody instance of the CPU restatement."""

    def __init__(self, cfg, _h=None):
        self.cfg = cfg
        self.N = int(cfg['num_nodes'])
        self.L = lib()
        if _h is not None:
            self.h = _h
        else:
            cc = make_c_config(cfg)
            self.h = C.c_void_p(self.L.orc_mpc_create(C.byref(cc)))

    def clone(self):
        return OracleMPC(self.cfg, _h=C.c_void_p(self.L.orc_mpc_clone(self.h)))

    def __del__(self):
        try:
            self.L.orc_mpc_destroy(self.h)
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.orc_mpc_error(self.h).decode())
        return rc

    def set_costs(self, des, Q, Phi, Phi_w):
        """AddQuadraticTrackingCost(des, Q), SetQuadraticFinalCost(Phi), SetLinearFinalCost(Phi_w): full 12 x 12 matrices, the final cost its own"""
        a = [np.ascontiguousarray(v, dtype=np.float64).reshape(k) for v, k in ((des, 12), (Q, 144), (Phi, 144), (Phi_w, 12))]
        self.L.orc_mpc_set_costs(self.h, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]))

    def set_warmstart(self, state13):
        s = np.ascontiguousarray(state13, dtype=np.float64)
        self.L.orc_mpc_set_warmstart(self.h, _d(s))

    def initial_run(self, state13, ee):
        s = np.ascontiguousarray(state13, dtype=np.float64)
        e = np.ascontiguousarray(ee, dtype=np.float64).reshape(-1)
        return self._chk(self.L.orc_mpc_initial_run(self.h, _d(s), _d(e)))

    def solve(self, state13, t, ee):
        s = np.ascontiguousarray(state13, dtype=np.float64)
        e = np.ascontiguousarray(ee, dtype=np.float64).reshape(-1)
        return self._chk(self.L.orc_mpc_solve(self.h, _d(s), t, _d(e)))

    def rti(self, state13, t, ee):
        s = np.ascontiguousarray(state13, dtype=np.float64)
        e = np.ascontiguousarray(ee, dtype=np.float64).reshape(-1)
        return self._chk(self.L.orc_mpc_rti(self.h, _d(s), t, _d(e)))

    def set_max_iter(self, it):
        self.L.orc_mpc_set_max_iter(self.h, int(it))

    def sizes(self):
        a = np.zeros(11, dtype=np.int32)
        self.L.orc_mpc_sizes(self.h, _i(a))
        keys = ['n', 'm', 'n_eq', 'n_ineq', 'n_force', 'n_pos', 'n_force_box', 'n_cone', 'n_ee_loc', 'n_td', 'n_start']
        return dict(zip(keys, [int(v) for v in a]))

    def x(self):
        a = np.zeros(self.sizes()['n'])
        self.L.orc_mpc_get_x(self.h, _d(a))
        return a

    def qp_x(self):
        a = np.zeros(self.sizes()['n'])
        self.L.orc_mpc_get_qp_x(self.h, _d(a))
        return a

    def z(self):
        a = np.zeros(self.sizes()['m'])
        self.L.orc_mpc_get_z(self.h, _d(a))
        return a

    def s(self):
        a = np.zeros(self.sizes()['m'])
        self.L.orc_mpc_get_s(self.h, _d(a))
        return a

    def states(self):
        a = np.zeros((self.N + 1, 13))
        self.L.orc_mpc_get_states(self.h, _d(a))
        return a

    def stats(self):
        a = np.zeros(12)
        self.L.orc_mpc_get_stats(self.h, _d(a))
        return dict(alpha=a[0], cost=a[1], eq_violation=a[2], step_norm=a[3], qp_iters=int(a[4]), status=int(a[5]),
                    res_primal=a[6], res_dual=a[7], gap_abs=a[8], gap_rel=a[9], box=(a[10], a[11]))

    def qp_dense(self):
        sz = self.sizes()
        n, m = sz['n'], sz['m']
        A = np.zeros((m, n)); b = np.zeros(m); P = np.zeros((n, n)); q = np.zeros(n)
        self.L.orc_mpc_get_qp_dense(self.h, _d(A), _d(b), _d(P), _d(q))
        return A, b, P, q

    def knots(self, ee):
        times = np.zeros(64); tt = np.zeros(64, np.int32)
        ft = np.zeros(3 * 64, np.int32); fv = np.zeros(3 * 64 * 2)
        pt = np.zeros(3 * 64, np.int32); pv = np.zeros(3 * 64 * 2)
        K = self.L.orc_mpc_get_knots(self.h, ee, _d(times), _i(tt), _i(ft), _d(fv), _i(pt), _d(pv))
        return dict(K=K, times=times[:K].copy(), ttypes=tt[:K].copy(), ftype=ft.reshape(3, 64)[:, :K].copy(),
                    fvals=fv.reshape(3, 64, 2)[:, :K].copy(), ptype=pt.reshape(3, 64)[:, :K].copy(),
                    pvals=pv.reshape(3, 64, 2)[:, :K].copy())

    def trajectory_record(self, host):
        """the oracle's current mpc::Trajectory as the product's flat record (host.Trajectory = srbm_trajectory): what a caller
        hands to MPC::SetWarmStartTrajectory.  Knot kind from (TimeType, force NodeType): LO 0, TD 1, stance-interior 2, mid-swing 3."""
        t = host.Trajectory()
        t.num_states = self.N + 1
        t.init_time = self.L.orc_mpc_init_time(self.h)
        t.node_dt = self.cfg['integrator_dt']; t.swing_height = self.cfg['swing_height']; t.foot_offset = self.cfg['foot_offset']
        st = self.states()
        for k in range(self.N + 1):
            for i in range(13):
                t.states[k][i] = st[k, i]
        for ee in range(4):
            kn = self.knots(ee)
            K = kn['K']
            assert K <= 32
            t.nk[ee] = K
            for k in range(K):
                tt, ft = int(kn['ttypes'][k]), int(kn['ftype'][0][k])
                kind = tt if tt < 2 else (2 if ft == 1 else 3)
                t.knot_kind[ee][k] = kind
                t.knot_time[ee][k] = kn['times'][k]
                for c in range(3):
                    t.force[ee][c][k][0] = kn['fvals'][c][k][0] if kind == 2 else 0.0
                    t.force[ee][c][k][1] = kn['fvals'][c][k][1] if kind == 2 else 0.0
                for c in range(2):
                    t.pos_xy[ee][c][k] = kn['pvals'][c][k][0] if kind <= 1 else 0.0
        return t

    def contact_times(self, ee):
        t = np.zeros(32); ty = np.zeros(32, np.int32)
        k = self.L.orc_mpc_get_contact_times(self.h, ee, _d(t), _i(ty))
        return t[:k].copy(), ty[:k].copy()

    def set_contact_times(self, times_per_ee):
        counts = np.array([len(t) for t in times_per_ee], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, float) for t in times_per_ee]))
        return self._chk(self.L.orc_mpc_set_contact_times(self.h, len(times_per_ee), _i(counts), _d(flat)))

    def adjust_for_current_contacts(self, t, in_contact):
        c = np.ascontiguousarray(in_contact, dtype=np.int32)
        return self._chk(self.L.orc_mpc_adjust_for_current_contacts(self.h, t, _i(c)))

    def ee_value(self, ee, is_position, coord, t):
        return self.L.orc_mpc_ee_value(self.h, ee, int(is_position), coord, t)

    def plant_integrate(self, state13, t, dt, num_steps, advance_time=0):
        """RKIntegrator::CalcIntegral (rk_integrator.cpp:14-30) under the current trajectory"""
        out = np.zeros(13)
        self._chk(self.L.orc_mpc_plant_integrate(self.h, _d(np.ascontiguousarray(state13, float)), t, dt,
                                                 int(num_steps), int(advance_time), _d(out)))
        return out

    # ---- bilevel step ----
    def gait_gradient(self):
        g = np.zeros(128)
        k = self.L.orc_gait_gradient(self.h, _d(g))
        if k == -2:
            raise RuntimeError(self.L.orc_mpc_error(self.h).decode())
        return None if k < 0 else g[:k].copy()

    def gait_d(self):
        sz = self.sizes()
        d = np.zeros(sz['n'] + sz['m'])
        self.L.orc_gait_get_d(self.h, _d(d))
        return d

    def param_partials(self, ee, idx, traj_src=None):
        sz = self.sizes()
        dA = np.zeros((sz['n_eq'], sz['n'])); dG = np.zeros((sz['n_ineq'], sz['n']))
        db = np.zeros(sz['n_eq']); dh = np.zeros(sz['n_ineq'])
        self._chk(self.L.orc_gait_param_partials(self.h, traj_src.h if traj_src is not None else None, ee, idx, _d(dA), _d(dG), _d(db), _d(dh)))
        return dA, dG, db, dh

    def gait_optimize(self, time):
        step = np.zeros(128); new = np.zeros(128)
        self._chk(self.L.orc_gait_optimize(self.h, time, _d(step), _d(new)))
        return step, new

    def gait_line_search(self, state13, t, ee):
        s = np.ascontiguousarray(state13, dtype=np.float64)
        e = np.ascontiguousarray(ee, dtype=np.float64).reshape(-1)
        costs = np.zeros(10)
        k = self._chk(self.L.orc_gait_line_search(self.h, _d(s), t, _d(e), _d(costs)))
        return k, costs

    def gait_line_search_with_quality(self, state13, t, ee):
        """-> (argmin, costs[10], mpc::SolveQuality of every candidate's solve)"""
        s = np.ascontiguousarray(state13, dtype=np.float64)
        e = np.ascontiguousarray(ee, dtype=np.float64).reshape(-1)
        costs = np.zeros(10); q = np.zeros(10, np.int32)
        k = self._chk(self.L.orc_gait_line_search_q(self.h, _d(s), t, _d(e), _d(costs), _i(q)))
        return k, costs, q



FEET0 = np.array([[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]], float)     # test/simulation_mpc.cpp:104-108


def first_rti_sizes(cfg, phase=None):
    """(n_u, wc, n_ineq) of the first RTI step from srb_init with the feet at FEET0: n_u = n - 12 (N + 1) spline variables, wc = n_force / 3 (the
    width of the compact dense rows, srbm_k3_lds.hiph), the inequality rows.  phase: after the cold start the contact times are set that far
    apart, as many per foot as the cold start has"""
    N = cfg['num_nodes']
    s0 = np.array(cfg['srb_init'], float)
    o = OracleMPC(cfg)
    o.set_warmstart(s0)
    o.initial_run(s0, FEET0)
    if phase is not None:
        o.set_contact_times([phase * np.arange(len(o.contact_times(e)[0])) for e in range(4)])
    o.rti(s0, 0.0, FEET0)
    sz = o.sizes()
    return sz['n'] - 12 * (N + 1), sz['n_force'] // 3, sz['n_ineq']

def qp_solve(P, q, A, b, cones, tol_gap=1e-8, tol_feas=1e-8):
    """cones: list of (is_nonneg, dim).  P dense symmetric, A dense."""
    L = lib()
    P = np.asarray(P, float); A = np.asarray(A, float)
    n, m = P.shape[0], A.shape[0]
    pr, pc = np.nonzero(np.triu(P)); pv = P[pr, pc]
    ar, ac = np.nonzero(A); av = A[ar, ac]
    pr = pr.astype(np.int32); pc = pc.astype(np.int32); ar = ar.astype(np.int32); ac = ac.astype(np.int32)
    pv = np.ascontiguousarray(pv); av = np.ascontiguousarray(av)
    q = np.ascontiguousarray(q, dtype=float); b = np.ascontiguousarray(b, dtype=float)
    cn = np.array([c[0] for c in cones], np.int32); cd = np.array([c[1] for c in cones], np.int32)
    x = np.zeros(n); z = np.zeros(m); s = np.zeros(m); it = C.c_int(0)
    st = L.orc_qp_solve(n, m, len(pv), _i(pr), _i(pc), _d(pv), _d(q), len(av), _i(ar), _i(ac), _d(av), _d(b), len(cones),
                        _i(cn), _i(cd), tol_gap, tol_feas, _d(x), _d(z), _d(s), C.byref(it))
    return dict(status=st, x=x, z=z, s=s, iters=it.value)


def qp_sensitivity(P, A_all, q, x, z, s, n_eq, n_ineq):
    L = lib()
    n = len(x)
    P = np.ascontiguousarray(P, dtype=float); A_all = np.ascontiguousarray(A_all, dtype=float)
    dA = np.zeros((n_eq, n)); dG = np.zeros((n_ineq, n)); dq = np.zeros(n); db = np.zeros(n_eq); dh = np.zeros(n_ineq)
    L.orc_qp_sensitivity(n, n_eq, n_ineq, _d(P), _d(A_all), _d(np.ascontiguousarray(q, dtype=float)),
                         _d(np.ascontiguousarray(x)), _d(np.ascontiguousarray(z)), _d(np.ascontiguousarray(s)),
                         _d(dA), _d(dG), _d(dq), _d(db), _d(dh))
    return dA, dG, dq, db, dh


class OracleSpline:
    FORCE, POSITION = 0, 1

    def __init__(self, times, start_in_contact, num_force_polys=3, _h=None):
        self.L = lib()
        if _h is not None:
            self.h = _h
        else:
            t = np.ascontiguousarray(times, dtype=float)
            self.h = C.c_void_p(self.L.orc_spline_create(len(t), _d(t), int(start_in_contact), num_force_polys))

    def clone(self):
        return OracleSpline(None, None, _h=C.c_void_p(self.L.orc_spline_clone(self.h)))

    def __del__(self):
        try:
            self.L.orc_spline_destroy(self.h)
        except Exception:
            pass

    def value_at(self, ty, coord, t):
        return self.L.orc_spline_value_at(self.h, ty, coord, t)

    def lin(self, ty, coord, t):
        out = np.zeros(8)
        k = self.L.orc_spline_lin(self.h, ty, coord, t, _d(out))
        if k < 0:
            raise RuntimeError('no mutable variables')
        return out[:k].copy()

    def vars_idx(self, ty, coord, t):
        idx = C.c_int(0)
        k = self.L.orc_spline_vars_idx(self.h, ty, coord, t, C.byref(idx))
        if k < 0:
            raise RuntimeError('no mutable variables')
        return idx.value, k

    def is_force_mutable(self, t):
        return bool(self.L.orc_spline_is_force_mutable(self.h, t))

    def add_poly(self, dt):
        self.L.orc_spline_add_poly(self.h, dt)

    def remove_poly(self, t):
        return self.L.orc_spline_remove_poly(self.h, t)

    def set_vars(self, ty, coord, node, a, b):
        rc = self.L.orc_spline_set_vars(self.h, ty, coord, int(node), a, b)
        if rc < 0:
            raise RuntimeError('set_vars failed')

    def mutable_nodes(self, ty, coord):
        out = np.zeros(128, np.int32)
        k = self.L.orc_spline_mutable_nodes(self.h, ty, coord, _i(out))
        return [int(v) for v in out[:k]]

    def times(self):
        out = np.zeros(128); ty = np.zeros(128, np.int32)
        k = self.L.orc_spline_times(self.h, _d(out), _i(ty))
        return out[:k].copy(), ty[:k].copy()

    def node_type(self, ty, coord, node):
        return self.L.orc_spline_node_type(self.h, ty, coord, node)

    def qp_vec(self, ty, coord):
        out = np.zeros(256)
        k = self.L.orc_spline_qp_vec(self.h, ty, coord, _d(out))
        return out[:k].copy()

    def end_time(self):
        return self.L.orc_spline_end_time(self.h)

    def start_time(self):
        return self.L.orc_spline_start_time(self.h)

    def contact_times(self):
        out = np.zeros(64)
        k = self.L.orc_spline_contact_times(self.h, _d(out))
        return out[:k].copy()

    def set_contact_times(self, t):
        t = np.ascontiguousarray(t, dtype=float)
        rc = self.L.orc_spline_set_contact_times(self.h, len(t), _d(t))
        if rc < 0:
            raise RuntimeError('set_contact_times failed %d' % rc)

    def partial_wrt_time(self, ty, coord, t, idx):
        return self.L.orc_spline_partial_wrt_time(self.h, ty, coord, t, idx)

    def coef_partial_wrt_time(self, ty, coord, t, idx, dtwdth=0.0):
        out = np.zeros(8)
        k = self.L.orc_spline_coef_partial_wrt_time(self.h, ty, coord, t, idx, dtwdth, _d(out))
        if k < 0:
            raise RuntimeError('coef partial failed')
        return out[:k].copy()
