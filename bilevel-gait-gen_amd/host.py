"""Python binding of the C-ABI in include/srbm_rti.h (libsrbm_rti.so, HIP/gfx950).

`BatchMPC` mirrors the public surface of the reference's mpc::MPCSingleRigidBody for a batch of instances
(/root/reference/mpc/include/mpc.h:70-170, mpc_single_rigid_body.h:11-76): same method names (snake_case), same
argument meaning.  There is NO CPU fallback: if the HIP library or a GPU is missing this module raises.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SRBM_RTI_LIB', os.path.join(HERE, 'libsrbm_rti.so'))   # override: A/B builds of scripts/dev_ab.py
# the LARGE-capacity build of the same sources (N <= 100, n_u <= 240, csrc/srbm_types.h): same C-ABI, slower (normal matrix in L2)
LIB_PATH_LARGE = os.environ.get('SRBM_RTI_LIB_LARGE', os.path.join(HERE, 'libsrbm_rti_large.so'))
CONFIG_DIR = os.path.join(HERE, 'configs')

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

SOLVE_QUALITY = ['Solved', 'SolvedInacc', 'MaxIter', 'PrimalInfeasible', 'DualInfeasible', 'PrimalInfeasibleInacc',
                 'DualInfeasibleInacc', 'Unsolved', 'Other']


class MPCInfo(C.Structure):          # srbm_mpc_info
    _fields_ = [('num_nodes', C.c_int), ('integrator_dt', C.c_double), ('friction_coef', C.c_double),
                ('force_bound', C.c_double), ('swing_height', C.c_double), ('foot_offset', C.c_double),
                ('ee_box_size', C.c_double * 2), ('force_cost', C.c_double)]


class WbcModel(C.Structure):         # srbm_wbc_model
    _fields_ = [('body_mass', C.c_double * 13), ('body_com', (C.c_double * 3) * 13), ('body_inertia', (C.c_double * 9) * 13),
                ('torque_bounds', C.c_double * 12), ('kp_joint_gains', C.c_double * 12), ('kd_joint_gains', C.c_double * 12),
                ('base_pos_gains', C.c_double * 2), ('base_ang_gains', C.c_double * 2),
                ('leg_tracking_weight', C.c_double), ('torso_tracking_weight', C.c_double), ('force_tracking_weight', C.c_double),
                ('friction_coef', C.c_double), ('max_grf', C.c_double)]


class Model(C.Structure):            # srbm_model
    _fields_ = [('mass', C.c_double), ('Ir', C.c_double * 9), ('hip_xy', C.c_double * 8)]


KMAX, NODES_MAX, RCCL_UNIQUE_ID_BYTES = 32, 101, 128       # SRBM_TRAJ_KMAX, SRBM_TRAJ_NODES_MAX, SRBM_RCCL_UNIQUE_ID_BYTES = sizeof(ncclUniqueId)
# srbm_set_solver_step_rule: a new batch runs every solve to the reference's gap criterion (0, 0); these are the values bench.py opts into for
# its headline line (include/srbm_rti.h: SRBM_FAST_TOL_STEP, SRBM_FAST_START_MU)
FAST_TOL_STEP, FAST_START_MU = 1e-5, 0.1
# srbm_wb_plant_set_terrain: the most patches per instance, the doubles of a patch (SRBM_TERRAIN_PATCHES, SRBM_TERRAIN_DOUBLES)
TERRAIN_PATCHES, TERRAIN_DOUBLES = 8, 8
# srbm_wb_plant_set_joints: the doubles of a joint, of an instance's stops and of its record (SRBM_JOINT_DOUBLES, _STOP_DOUBLES, _RECORD_DOUBLES)
JOINT_DOUBLES, JOINT_STOP_DOUBLES, JOINT_RECORD_DOUBLES = 8, 2, 8
# srbm_set_solver_tolerances(gap_abs, gap_rel, feas, max_iter): ClarabelInterface's settings (clarabel_interface.cpp:165-175), which are also what
# a new batch holds (srbm_batch_create).  srbm_loader re-exports the name as workloads.REFERENCE_SOLVER_SETTINGS
REFERENCE_SOLVER_SETTINGS = (1e-15, 1e-15, 1e-10, 200)


class Trajectory(C.Structure):       # srbm_trajectory: mpc::Trajectory as a flat record (include/srbm_rti.h)
    _fields_ = [('num_states', C.c_int), ('nk', C.c_int * 4), ('knot_kind', (C.c_int * KMAX) * 4),
                ('init_time', C.c_double), ('node_dt', C.c_double), ('swing_height', C.c_double), ('foot_offset', C.c_double),
                ('states', (C.c_double * 13) * NODES_MAX), ('knot_time', (C.c_double * KMAX) * 4),
                ('force', (((C.c_double * 2) * KMAX) * 3) * 4), ('pos_xy', ((C.c_double * KMAX) * 2) * 4)]

    # ---- the part of mpc::Trajectory's interface the caller uses (controllers/mpc_controller.cpp:171-186,415-509) ----
    def get_time(self, node):                      # Trajectory::GetTime (trajectory.cpp:412-414)
        return self.init_time + self.node_dt * node

    def get_node(self, time):                      # Trajectory::GetNode (trajectory.cpp:479-481)
        return int(np.ceil((time - self.init_time) / self.node_dt))

    def get_states(self):
        return np.ctypeslib.as_array(self.states)[:self.num_states].copy()

    def _eval(self, ee, time):
        f = (C.c_double * 3)(); p = (C.c_double * 3)(); c = C.c_int(0)
        rc = lib().srbm_trajectory_eval(C.byref(self), int(ee), time, f, p, C.byref(c))
        if rc != 0:
            raise RuntimeError('trajectory lookup failed at t=%g (error bits %d)' % (time, rc))   # the reference throws std::runtime_error
        return np.array(f[:]), np.array(p[:]), bool(c.value)

    def get_force(self, ee, time):                 # Trajectory::GetForce (trajectory.cpp:395-402)
        return self._eval(ee, time)[0]

    def get_end_effector_location(self, ee, time):     # Trajectory::GetEndEffectorLocation (trajectory.cpp:404-410)
        return self._eval(ee, time)[1]

    def get_contacts(self, time):                  # Trajectory::GetContacts
        return [self._eval(ee, time)[2] for ee in range(4)]

    def get_contact_times(self):                   # Trajectory::GetContactTimes: per foot the times of the LO / TD knots
        out = []
        for ee in range(4):
            out.append([self.knot_time[ee][k] for k in range(self.nk[ee]) if self.knot_kind[ee][k] <= 1])
        return out


# ---- the prototype of every exported function, and the one place that types the binding ----
# C type -> ctypes type, `const` left out.  A host array is a typed pointer: a pointer to another element type or a bare integer is refused before
# the call.  Handles, void* and DEVICE pointers (`dev*`: the *_dev parameters of the header, whatever they point to) are c_void_p: integer addresses.
C_TYPES = {
    'void': None, 'int': C.c_int, 'double': C.c_double, 'long': C.c_long, 'char*': C.c_char_p, 'char**': C.POINTER(C.c_char_p),
    'double*': _dp, 'int*': _ip, 'long long*': C.POINTER(C.c_longlong),
    'srbm_batch*': C.c_void_p, 'srbm_gait*': C.c_void_p, 'ncclComm_t': C.c_void_p, 'void*': C.c_void_p, 'dev*': C.c_void_p,
    'srbm_batch**': C.POINTER(C.c_void_p), 'srbm_gait**': C.POINTER(C.c_void_p), 'ncclComm_t*': C.POINTER(C.c_void_p),
    'srbm_mpc_info*': C.POINTER(MPCInfo), 'srbm_model*': C.POINTER(Model), 'srbm_wbc_model*': C.POINTER(WbcModel), 'srbm_trajectory*': C.POINTER(Trajectory),
    'srbm_leg_kinematics*': _dp,         # no mirror: its one member double origin[4][4][3] is passed as a flat array
}


def prototypes(text, types=C_TYPES):
    """name -> (restype, argtypes) from lines `ret name(type, type, ...)` spelled with the keys of `types`"""
    table = {}
    for line in text.strip().split('\n'):
        head, args = line.strip().rstrip(')').split('(')
        ret, name = head.rsplit(None, 1)
        table[name] = (types[ret], tuple(types[a.strip()] for a in args.split(',') if a.strip()))
    return table


def declare(L, table):
    """set restype and argtypes of every function of `table` on the loaded library L; the only place that sets either"""
    for name, (restype, argtypes) in table.items():
        f = getattr(L, name)                # AttributeError ('undefined symbol') if the library lacks it
        f.restype, f.argtypes = restype, argtypes
    return L


# include/srbm_rti.h, then the srbm_debug_* hooks that only csrc/srbm_capi.hip declares (tests/test_abi_prototypes.py holds both to the C text and to
# the symbols of the two libraries)
PROTOTYPES = prototypes('''\
int srbm_batch_create(srbm_batch**, int, srbm_mpc_info*, srbm_model*, int)
int srbm_batch_create_each(srbm_batch**, int, srbm_mpc_info*, srbm_model*, int)
int srbm_get_instance_model(srbm_batch*, int, srbm_mpc_info*, srbm_model*)
int srbm_batch_destroy(srbm_batch*)
char* srbm_last_error()
int srbm_batch_clone(srbm_batch*, srbm_batch**)
int srbm_batch_size(srbm_batch*)
int srbm_get_capacity(int*)
int srbm_num_nodes(srbm_batch*)
int srbm_add_quadratic_tracking_cost(srbm_batch*, double*, double*)
int srbm_set_quadratic_final_cost(srbm_batch*, double*)
int srbm_set_linear_final_cost(srbm_batch*, double*)
int srbm_add_force_cost(srbm_batch*, double)
int srbm_add_quadratic_tracking_cost_each(srbm_batch*, int, int, double*, double*)
int srbm_set_quadratic_final_cost_each(srbm_batch*, int, int, double*)
int srbm_set_linear_final_cost_each(srbm_batch*, int, int, double*)
int srbm_add_force_cost_each(srbm_batch*, int, int, double*)
int srbm_set_state_trajectory_warm_start(srbm_batch*, double*)
int srbm_set_solver_tolerances(srbm_batch*, double, double, double, int)
int srbm_set_solver_step_rule(srbm_batch*, double, double)
int srbm_get_solver_step_rule(srbm_batch*, double*, double*)
int srbm_get_solve_flags(srbm_batch*, int*)
int srbm_create_initial_run(srbm_batch*, double*, double*)
int srbm_get_real_time_update(srbm_batch*, double*, double*, double*)
int srbm_get_real_time_update_dev(srbm_batch*, dev*, dev*, dev*)
int srbm_rti_advance(srbm_batch*, int, int)
int srbm_rti_advance_unfused(srbm_batch*, int, int)
int srbm_plant_set_state(srbm_batch*, double*)
int srbm_plant_get_state(srbm_batch*, double*)
int srbm_plant_set_push(srbm_batch*, double*, double*)
int srbm_plant_set_period(srbm_batch*, double*)
int srbm_plant_get_period(srbm_batch*, double*)
int srbm_closed_loop_advance(srbm_batch*, int, int, int, int)
int srbm_plant_advance(srbm_batch*, int, int, int, double*, double*, double*)
int srbm_synchronize(srbm_batch*)
void* srbm_stream(srbm_batch*)
int srbm_step_log_record_doubles()
int srbm_step_log_enable(srbm_batch*, int)
int srbm_step_log_reset(srbm_batch*)
int srbm_step_log_count(srbm_batch*, int*)
int srbm_step_log_get(srbm_batch*, int, int, double*)
int srbm_step_log_copy_dev(srbm_batch*, int, int, dev*)
int srbm_rollout_summary_doubles()
int srbm_rollout_summary_enable(srbm_batch*, double*, double*)
int srbm_rollout_summary_reset(srbm_batch*)
int srbm_rollout_summary_fold(srbm_batch*, int, int)
int srbm_rollout_summary_get(srbm_batch*, int, int, double*)
int srbm_rollout_summary_copy_dev(srbm_batch*, dev*)
int srbm_rollout_study(srbm_batch*, double*)
int srbm_rollout_study_dev(srbm_batch*, dev*, int, dev*)
int srbm_rollout_fold_host(double*, int, int, int, int, double*, double*, double*, double*)
int srbm_rollout_study_host(double*, int, double*)
int srbm_sizeof_trajectory()
int srbm_get_trajectory(srbm_batch*, int, int, srbm_trajectory*)
int srbm_set_warm_start_trajectory(srbm_batch*, int, int, srbm_trajectory*)
int srbm_trajectory_eval(srbm_trajectory*, int, double, double*, double*, int*)
int srbm_trajectory_splines_as_vec(srbm_trajectory*, double*, int, int*, int*)
int srbm_convert_manifold_to_tangent(double*, double*)
int srbm_convert_tangent_to_manifold(double*, double*)
int srbm_eval_trajectory(srbm_batch*, double*, double*, double*, int*)
int srbm_eval_trajectory_dev(srbm_batch*, dev*, dev*, dev*, dev*)
int srbm_get_ee_box_center(srbm_batch*, double*)
int srbm_get_cost(srbm_batch*, double*)
int srbm_get_avg_cost(srbm_batch*, double*)
int srbm_get_merit(srbm_batch*, double*, double*)
int srbm_update_contact_times(srbm_batch*, double*, int)
int srbm_adjust_for_current_contacts(srbm_batch*, double*, int*)
int srbm_gait_create(srbm_batch*, srbm_gait**)
int srbm_gait_destroy(srbm_gait*)
int srbm_gait_set_contact_times_from_trajectory(srbm_gait*)
int srbm_gait_get_contact_times(srbm_gait*, double*, int*)
int srbm_gait_compute_sensitivity(srbm_gait*)
int srbm_gait_get_sensitivity(srbm_gait*, double*, int)
int srbm_gait_compute_gradient(srbm_gait*)
int srbm_gait_get_gradient(srbm_gait*, double*, int*)
int srbm_gait_set_gradient(srbm_gait*, double*, int*)
int srbm_gait_get_param_partials(srbm_batch*, int, int, int, double*, double*, double*, double*)
int srbm_gait_optimize_contact_times(srbm_gait*, double*)
int srbm_gait_get_lp_result(srbm_gait*, int*, double*)
int srbm_gait_set_step(srbm_gait*, double*)
int srbm_gait_get_step(srbm_gait*, double*)
int srbm_gait_line_search(srbm_gait*, double*, double*, double*, int*, double*)
int srbm_gait_rti_advance(srbm_gait*, int, int, int)
int srbm_gait_closed_loop_advance(srbm_gait*, int, int, int, int, int)
int srbm_gait_get_line_search_result(srbm_gait*, int*, double*)
int srbm_gait_get_candidate_status(srbm_gait*, int*, int*)
srbm_batch* srbm_gait_debug_candidates(srbm_gait*)
int srbm_set_leg_kinematics(srbm_batch*, srbm_leg_kinematics*)
int srbm_forward_kinematics(srbm_batch*, double*, double*)
int srbm_inverse_kinematics(srbm_batch*, double*, double*, double*, double*, int*, int*)
int srbm_get_targets_from_traj(srbm_batch*, double*, double*, double*, double*, int*)
int srbm_get_targets_from_traj_dev(srbm_batch*, dev*, dev*, dev*, dev*, dev*)
int srbm_set_wbc_model(srbm_batch*, srbm_wbc_model*)
int srbm_qp_control(srbm_batch*, double*, double*, int*, double*, double*, double*, double*, double*, int*, double*)
int srbm_qp_control_dev(srbm_batch*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_control_tick_reset(srbm_batch*, double*)
int srbm_control_tick(srbm_batch*, double*, double*, double*, double*, double*, int*, double*, double*, int*, double*, double*)
int srbm_control_tick_dev(srbm_batch*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_wb_plant_set_state(srbm_batch*, double*, double*)
int srbm_wb_plant_get_state(srbm_batch*, double*, double*)
int srbm_wb_plant_step_dev(srbm_batch*, int, double, dev*, dev*, dev*, dev*)
int srbm_controller_advance(srbm_batch*, int, int, int, double)
int srbm_tick_log_record_doubles()
int srbm_tick_log_enable(srbm_batch*, int)
int srbm_tick_log_reset(srbm_batch*)
int srbm_tick_log_count(srbm_batch*, int*)
int srbm_tick_log_get(srbm_batch*, int, int, double*)
int srbm_tick_log_copy_dev(srbm_batch*, int, int, dev*)
int srbm_tick_summary_doubles()
int srbm_tick_summary_enable(srbm_batch*, double*, double*)
int srbm_tick_summary_reset(srbm_batch*)
int srbm_tick_summary_fold(srbm_batch*, int, int)
int srbm_tick_summary_fold_dev(srbm_batch*, dev*, int, int, int)
int srbm_tick_summary_get(srbm_batch*, int, int, double*)
int srbm_tick_summary_copy_dev(srbm_batch*, dev*)
int srbm_tick_study(srbm_batch*, double*)
int srbm_tick_study_dev(srbm_batch*, dev*, int, dev*)
int srbm_tick_fold_host(double*, int, int, int, int, double*, double*, double*)
int srbm_tick_study_host(double*, int, double*)
int srbm_wb_plant_set_kind(srbm_batch*, int)
int srbm_wb_plant_set_actuators(srbm_batch*, double*, double*, double*, int)
int srbm_wb_plant_set_bodies_each(srbm_batch*, double*, double*, double*)
int srbm_wb_forward_dynamics(srbm_batch*, double*, double*, double*, int*, double*, int*)
int srbm_wb_forward_dynamics_dev(srbm_batch*, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_wb_fd_step_dev(srbm_batch*, int, double, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_wb_plant_set_ground(srbm_batch*, double*)
int srbm_wb_plant_set_terrain(srbm_batch*, double*, int)
int srbm_wb_plant_set_joints(srbm_batch*, double*, double*)
int srbm_wb_plant_get_joints(srbm_batch*, double*, double*)
int srbm_wb_plant_get_joint_state(srbm_batch*, double*)
int srbm_wb_plant_set_joint_state(srbm_batch*, double*)
int srbm_wb_plant_get_joint_record(srbm_batch*, double*)
int srbm_joint_law_host(int, int, double, double*, double*, double*, int*, double*, double*, double*, double*, double*)
int srbm_wb_plant_set_wrenches(srbm_batch*, double*, int)
int srbm_wb_plant_get_wrenches(srbm_batch*, double*, int*)
int srbm_wb_plant_get_wrench_record(srbm_batch*, double*)
int srbm_wb_wrench_force(srbm_batch*, double*, double*, double*, int*)
int srbm_wb_wrench_force_dev(srbm_batch*, dev*, dev*, dev*, dev*)
int srbm_wrench_active_host(int, double*, int, int, int, double, int, int*)
int srbm_wb_plant_get_contact_state(srbm_batch*, double*)
int srbm_wb_plant_set_contact_state(srbm_batch*, double*)
int srbm_wb_ground_dynamics(srbm_batch*, double*, double*, double*, double*, double*, double*, int*)
int srbm_wb_ground_dynamics_dev(srbm_batch*, dev*, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_wb_ground_step_dev(srbm_batch*, int, double, dev*, dev*, dev*, dev*, dev*, dev*)
int srbm_controller_set_contact_feedback(srbm_batch*, int)
int srbm_controller_get_contact_feedback(srbm_batch*, double*)
int srbm_controller_contact_feedback_dev(srbm_batch*, dev*, dev*)
int srbm_command_event_doubles()
int srbm_command_record_doubles()
int srbm_controller_set_commands(srbm_batch*, double*, int)
int srbm_controller_get_commands(srbm_batch*, double*, int*)
int srbm_controller_get_command_state(srbm_batch*, double*)
int srbm_controller_set_command_state(srbm_batch*, double*)
int srbm_controller_get_command_record(srbm_batch*, double*)
int srbm_controller_get_command_costs(srbm_batch*, double*, double*)
int srbm_controller_command_dev(srbm_batch*, dev*, dev*)
int srbm_command_target_host(int, double*, int, double*, double*, int, double*, double*, double*, double*, double*, double*, double*)
int srbm_gait_controller_advance(srbm_gait*, int, int, int, double, int)
int srbm_controller_set_latency(srbm_batch*, double*)
int srbm_controller_get_latency_record(srbm_batch*, double*)
int srbm_controller_get_published(srbm_batch*, int, int, srbm_trajectory*)
int srbm_controller_publish_dev(srbm_batch*, dev*, int, double, int)
int srbm_latency_publish_ticks_host(int, int, int, int, double, double*, int*, int, int*, int*)
int srbm_controller_set_sensors(srbm_batch*, double*, long long*)
int srbm_controller_get_sensors(srbm_batch*, double*, long long*)
int srbm_controller_get_sensor_state(srbm_batch*, double*)
int srbm_controller_set_sensor_state(srbm_batch*, double*)
int srbm_controller_get_sensor_record(srbm_batch*, double*)
int srbm_controller_get_measured(srbm_batch*, double*, double*)
int srbm_controller_measure_dev(srbm_batch*, int, double, dev*, dev*, dev*, dev*)
int srbm_sensor_philox_host(int*, int*, int*)
int srbm_sensor_state_init_host(int, double*, double*, double*)
int srbm_sensor_measure_host(int, int, int, double, double*, long long*, double*, double*, double*, double*, double*, double*)
int srbm_get_sizes(srbm_batch*, int*)
int srbm_get_status(srbm_batch*, int*, int*)
int srbm_get_status_accumulated(srbm_batch*, int*)
int srbm_clear_status_accumulators(srbm_batch*)
int srbm_get_solver_counters(srbm_batch*, long long*)
int srbm_get_stats(srbm_batch*, double*)
int srbm_get_qp_cost(srbm_batch*, double*)
int srbm_get_qp_solution(srbm_batch*, double*, int)
int srbm_get_raw_qp_minimiser(srbm_batch*, double*, int)
int srbm_get_dual_solution(srbm_batch*, double*, double*, int)
int srbm_get_trajectory_states(srbm_batch*, double*)
int srbm_get_knots(srbm_batch*, int, double*, int*, int*, double*, double*, double*)
int srbm_export_qp(srbm_batch*, int, double*, double*, double*, double*)
int srbm_result_record_doubles(int)
int srbm_pack_results_dev(srbm_batch*, dev*, int)
int srbm_pack_results(srbm_batch*, double*, int)
int srbm_allgather_results(srbm_batch*, ncclComm_t, dev*)
int srbm_rollout_allgather_dev(srbm_batch*, ncclComm_t, dev*)
int srbm_tick_summary_allgather_dev(srbm_batch*, ncclComm_t, dev*)
int srbm_rccl_get_unique_id(void*)
int srbm_rccl_comm_init_rank(srbm_batch*, int, int, void*, ncclComm_t*)
int srbm_rccl_comm_destroy(ncclComm_t)
int srbm_enable_kernel_timing(srbm_batch*, int)
int srbm_get_kernel_timing(srbm_batch*, double*, int*)
int srbm_get_kernel_timings(srbm_batch*, double*, int, int*)
int srbm_get_work_counters(srbm_batch*, double*, double*)
int srbm_get_executed_mfma(srbm_batch*, double*)
long srbm_bytes_per_instance()
int srbm_debug_get_profile(srbm_batch*, int, double*)
int srbm_debug_profile_slot(int, char**, char**)
int srbm_debug_trace_field(int, char**, int*)
int srbm_debug_solve_mapped(int, int, int*, int, double*, double*, double*, int*, double)
int srbm_debug_solve(int, int, double*, double*, double*, double*, int*, double)
int srbm_debug_cholesky(int, int, double*, double*, int*, double)
int srbm_debug_sym_matvec(int, int, double*, double*, double*)
int srbm_debug_hmatvec(int, int, double*, double*, double*)
int srbm_debug_dense_row_placement(int, int, int, int*)
int srbm_debug_h_stage(int, int, double*, double*, int, int, int, int*)
int srbm_debug_lds_base(int, int, int*)
int srbm_debug_get_trace(srbm_batch*, int, double*)
int srbm_debug_get_spline_step(srbm_batch*, int, double*, double*, int*, int*)
int srbm_debug_get_instance_iters(srbm_batch*, double*)
int srbm_debug_get_launch_info(srbm_batch*, int*)
int srbm_debug_get_condensed(srbm_batch*, int, double*, double*, double*, double*, int*, int*)''')


def build(force=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU).  Serialised by a file lock: the ranks of a multi-GPU run that
    find a library missing (a fresh box) must not run `make` on the same tree at the same time."""
    if force or not (os.path.exists(LIB_PATH) and os.path.exists(LIB_PATH_LARGE)):
        import fcntl
        with open(os.path.join(HERE, 'csrc', '.build.lock'), 'w') as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            try:
                subprocess.check_call(['make', '-s', '-j2', '-C', os.path.join(HERE, 'csrc')])
            finally:
                fcntl.flock(lk, fcntl.LOCK_UN)
    return LIB_PATH


_libs = {}


def lib(large=False):
    path = LIB_PATH_LARGE if large else LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError('%s is not built (run __graft_entry__.build()); there is no CPU fallback' % os.path.basename(path))
        L = declare(C.CDLL(path), PROTOTYPES)
        cap = (C.c_int * 4)()
        L.srbm_get_capacity(cap)
        L.capacity = dict(N=cap[0], nu=cap[1], samples=cap[2], knots=cap[3])
        L.Trajectory = Trajectory          # the record type, for the modules beside this one that do not import it (controller_rollout.published)
        _libs[path] = L
    return _libs[path]


def load_config(name='a1_configuration', **overrides):
    cfg = json.load(open(os.path.join(CONFIG_DIR, name + '.json')))
    cfg.update(overrides)
    return cfg


def load_yaml_config(yaml_path, model_constants):
    """The reference's own configuration files (apps/*.yaml, keys as parsed in /root/reference/test/simulation_mpc.cpp:55-89
    and controllers/mpc_controller.cpp:27-67) -> the cfg dict of BatchMPC.  model_constants: dict with 'mass', 'Ir' (3x3)
    and 'hip_xy' (FL FR RL RR) -- what the reference asks pinocchio for at construction."""
    import yaml
    y = yaml.safe_load(open(yaml_path))
    keys = ['num_nodes', 'integrator_dt', 'friction_coef', 'force_bound', 'swing_height', 'foot_offset', 'ee_box_size', 'force_cost',
            'Q_srbd_diag', 'srb_init']
    missing = [k for k in keys if k not in y]
    if missing:
        raise KeyError('%s: missing keys %s' % (yaml_path, missing))
    cfg = {k: y[k] for k in keys}
    if 'srb_target' in y:
        cfg['srb_target'] = y['srb_target']
    else:       # configurations that predate srb_target give x_des / y_des (apps/a1_gait_opt_config.yaml:126-129)
        tgt = list(y['srb_init']); tgt[0] = y.get('x_des', tgt[0]); tgt[1] = y.get('y_des', tgt[1]); cfg['srb_target'] = tgt
    cfg['gait_opt_freq'] = y.get('gait_opt_freq', 5)
    cfg['mass'] = float(model_constants['mass'])
    cfg['Ir'] = np.asarray(model_constants['Ir'], float).reshape(3, 3).tolist()
    cfg['hip_xy'] = np.asarray(model_constants['hip_xy'], float).reshape(4, 2).tolist()
    cfg['source'] = os.path.basename(yaml_path)
    return cfg


SOLVE_TYPE_NAMES = {0: 'Solved', 1: 'Solved Inacc', 2: 'Max Iter', 3: 'P - Infeasible', 4: 'D - Infeasible', 5: 'P - Infeasible Inacc',
                    6: 'D - Infeasible Inacc', 7: 'Unsolved'}      # MPC::PrintStatLineToFile, mpc.cpp:944-972


# One record of the step log (include/srbm_rti.h: srbm_step_log_*): field name -> slice of its STEP_LOG_DOUBLES doubles; [58, 64) is written by
# srbm_gait_closed_loop_advance alone (gait_rollout.GAIT_LOG_FIELDS) and 0 from every other entry
STEP_LOG_DOUBLES = 64
STEP_LOG_FIELDS = {
    'solve_number': slice(0, 1), 'init_time': slice(1, 2), 'status': slice(2, 3), 'err': slice(3, 4), 'solve_flags': slice(4, 5),
    'n': slice(5, 6), 'm': slice(6, 7), 'stats': slice(7, 15), 'qp_cost': slice(15, 16), 'merit_dd': slice(16, 17),
    'state': slice(17, 30), 'ee': slice(30, 42), 'force': slice(42, 54), 'in_contact': slice(54, 58)}
MERIT_MU = 5000.0        # MPC::GetMeritValue (mpc.cpp:749-753); the library's srbm_get_merit uses the same constant


def format_stat_line(solve_number, time_ms, stats, merit, merit_dd, status):
    """one table row of MPC::PrintStatLineToFile (mpc.cpp:974-989) from the values of one solve; stats as srbm_get_stats"""
    cw = 15
    s = stats
    vals = ['%d' % solve_number, '%g' % time_ms, '%g' % s[2], '%g' % s[3], '%g' % s[0], '%g' % s[1], '%g' % merit, '%g' % merit_dd,
            SOLVE_TYPE_NAMES.get(int(status), 'Other'), '%g' % s[1]]       # last column: cost_ = GetCostValue(prev_qp_sol), the same value as 'Cost' (mpc.cpp:809, msrb.cpp:183-184)
    return ''.join(v.ljust(cw) for v in vals) + '\n'


def step_log_merit(record):
    """the 'Merit' column of a step-log record (or an array of them): cost + mu * defect, formed as srbm_get_merit forms it"""
    record = np.asarray(record)
    return record[..., 8] + MERIT_MU * record[..., 9]


def stat_line_from_log(fh, record, time_ms):
    """the row print_stat_line writes after a one-step launch, from one step-log record [STEP_LOG_DOUBLES] of that solve"""
    r = np.asarray(record, dtype=np.float64)
    fh.write(format_stat_line(int(r[0]), time_ms, r[STEP_LOG_FIELDS['stats']], step_log_merit(r), r[16], r[2]))


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def quat_log3(q):
    """log of a unit quaternion (xyzw) -- closed form of pinocchio::quaternion::log3"""
    v = np.asarray(q[:3], float)
    n = np.linalg.norm(v)
    w = q[3]
    if n < 1e-8:
        return (2.0 / w) * (1.0 - n * n / (3.0 * w * w)) * v
    th = 2.0 * np.arctan2(n, w) if w >= 0 else -2.0 * np.arctan2(n, -w)
    return th / n * v


def manifold_to_tangent(s13):
    """SingleRigidBodyModel::ConvertManifoldStateToTangentState through the library's own host function (srbm_convert_manifold_to_tangent: no GPU
    needed), so that a Python caller and a C++ caller of the facade hand the MPC the same bits"""
    a = np.ascontiguousarray(s13, dtype=np.float64)
    t = np.zeros(12)
    if lib().srbm_convert_manifold_to_tangent(_d(a), _d(t)) != 0:
        raise RuntimeError('srbm: ' + lib().srbm_last_error().decode())
    return t


def _info_model(cfg):
    """the constructor data of one reference object: (srbm_mpc_info, srbm_model) of a cfg dict"""
    info = MPCInfo()
    info.num_nodes = int(cfg['num_nodes'])
    info.integrator_dt = cfg['integrator_dt']
    info.friction_coef = cfg['friction_coef']
    info.force_bound = cfg['force_bound']
    info.swing_height = cfg['swing_height']
    info.foot_offset = cfg['foot_offset']
    info.ee_box_size[:] = [float(v) for v in cfg['ee_box_size']]
    info.force_cost = cfg['force_cost']
    model = Model()
    model.mass = cfg['mass']
    model.Ir[:] = list(np.asarray(cfg['Ir'], float).reshape(-1))
    model.hip_xy[:] = list(np.asarray(cfg['hip_xy'], float).reshape(-1))
    return info, model


def _tracking_cost(cfg):
    """(Q, state_des) of the caller's cost set-up: /root/reference/controllers/mpc_controller.cpp:57-67"""
    return np.diag(np.asarray(cfg['Q_srbd_diag'], float)), manifold_to_tangent(cfg['srb_target'])


# keys of a cfg that are one value for the whole batch (srbm_batch_create_each; the leg kinematics and the whole-body QP model are batch-wide setters)
BATCH_WIDE_KEYS = ('num_nodes', 'integrator_dt', 'swing_height', 'foot_offset', 'hip_xy', 'large', 'leg_origins', 'body_model', 'torque_bounds',
                   'kp_joint_gains', 'kd_joint_gains', 'base_pos_gains', 'base_ang_gains', 'leg_tracking_weight', 'torso_tracking_weight',
                   'force_tracking_weight')


def _same(a, b):
    try:
        return np.array_equal(np.asarray(a, float), np.asarray(b, float))
    except (TypeError, ValueError):
        return a == b


class BatchMPC:
    """batch x mpc::MPCSingleRigidBody on one MI355X."""

    def __init__(self, cfg, batch, device=0, large=None, _cfgs=None):
        self.N = int(cfg['num_nodes'])
        # horizons beyond the standard build's 50 nodes (or an explicit request) go to the LARGE-capacity build
        self.large = bool(cfg.get('large', self.N > lib().capacity['N'])) if large is None else bool(large)
        self.L = lib(self.large)
        self.NUMAX, self.NSMAX = self.L.capacity['nu'], self.L.capacity['samples']
        self.cfg = cfg
        self.batch = int(batch)
        self.h = C.c_void_p()
        if _cfgs is None:
            info, model = _info_model(cfg)
            self._chk(self.L.srbm_batch_create(C.byref(self.h), self.batch, C.byref(info), C.byref(model), int(device)))
            Q, des = _tracking_cost(cfg)
            self.add_quadratic_tracking_cost(des, Q)
            self.set_quadratic_final_cost(Q)
            self.set_linear_final_cost(-1 * Q @ des)
        else:
            im = [_info_model(c) for c in _cfgs]
            infos = (MPCInfo * self.batch)(*[i for i, _ in im]); models = (Model * self.batch)(*[m for _, m in im])
            self._chk(self.L.srbm_batch_create_each(C.byref(self.h), self.batch, infos, models, int(device)))
            qd = [_tracking_cost(c) for c in _cfgs]
            Q = np.stack([q for q, _ in qd]); des = np.stack([d for _, d in qd])
            self.add_quadratic_tracking_cost_each(0, des, Q)
            self.set_quadratic_final_cost_each(0, Q)
            self.set_linear_final_cost_each(0, np.stack([-1 * q @ d for q, d in qd]))      # (the expression of the uniform path, per instance)
        if 'leg_origins' in cfg:            # leg geometry for the whole-body targets (row f3)
            lo = np.ascontiguousarray(cfg['leg_origins'], dtype=np.float64).reshape(4, 4, 3)
            self._chk(self.L.srbm_set_leg_kinematics(self.h, _d(lo)))
        if 'body_model' in cfg and 'torque_bounds' in cfg:        # whole-body QP of the low-level controller (row f3)
            w = WbcModel()
            for b, body in enumerate(cfg['body_model']):
                w.body_mass[b] = body['mass']
                w.body_com[b][:] = body['com']
                w.body_inertia[b][:] = list(np.asarray(body['inertia'], float).reshape(-1))
            w.torque_bounds[:] = [float(x) for x in cfg['torque_bounds']]
            w.kp_joint_gains[:] = [float(x) for x in cfg['kp_joint_gains']]; w.kd_joint_gains[:] = [float(x) for x in cfg['kd_joint_gains']]
            w.base_pos_gains[:] = [float(x) for x in cfg['base_pos_gains']]; w.base_ang_gains[:] = [float(x) for x in cfg['base_ang_gains']]
            w.leg_tracking_weight = cfg['leg_tracking_weight']; w.torso_tracking_weight = cfg['torso_tracking_weight']
            w.force_tracking_weight = cfg['force_tracking_weight']; w.friction_coef = cfg['friction_coef']; w.max_grf = cfg['force_bound']
            self._chk(self.L.srbm_set_wbc_model(self.h, C.byref(w)))

    @classmethod
    def from_configs(cls, cfgs, device=0, large=None):
        """One instance per cfg dict, each its own reference object: its own MPCInfo, mass and inertia (srbm_batch_create_each) and its own
        tracking cost from its Q_srbd_diag / srb_target, set up as BatchMPC(cfg, 1) sets it (mpc_controller.cpp:57-67).  The horizon, the time step,
        the foot geometry, the leg kinematics and the whole-body QP model (set from config 0) are batch-wide: configs that differ in one raise
        ValueError before the library is called."""
        cfgs = list(cfgs)
        if not cfgs:
            raise ValueError('from_configs: no configs')
        c0 = cfgs[0]
        for i, c in enumerate(cfgs[1:], 1):
            for k in BATCH_WIDE_KEYS:
                if (k in c) != (k in c0) or (k in c and not _same(c[k], c0[k])):
                    raise ValueError('from_configs: config %d: %s differs from config 0 (it is batch-wide: one value for every instance)' % (i, k))
        return cls(c0, len(cfgs), device=device, large=large, _cfgs=cfgs)

    @classmethod
    def cold_start(cls, cfg, states, ees, mode=None, large=None, device=0, initial_run=True):
        """The cold start of the tests and the developer scripts in one call: a batch of len(states) instances of cfg (a list of cfgs: from_configs),
        warm-started at `states`, at the reference's solver settings, with the step rule `mode` = (tol_step, start_mu) (None: a new batch keeps
        the library's (0, 0)), after create_initial_run(states, ees) unless initial_run is false.  The three setters write disjoint fields, so a
        caller that needs something between them and the initial run passes initial_run=False and goes on from there.  (bench.py does not use
        this: it keeps its own three copies of the sequence, so that what it measures is written out in the file that measures it.)"""
        if isinstance(cfg, (list, tuple)):
            g = cls.from_configs(cfg, device=device, large=large)
        else:
            g = cls(cfg, len(np.asarray(states, dtype=np.float64).reshape(-1, 13)), device=device, large=large)
        g.set_state_trajectory_warm_start(states)
        g.set_solver_tolerances(*REFERENCE_SOLVER_SETTINGS)
        if mode is not None:
            g.set_solver_step_rule(*mode)
        if initial_run:
            g.create_initial_run(states, ees)
        return g

    def instance_model(self, inst):
        """srbm_get_instance_model: (srbm_mpc_info, srbm_model) of instance inst"""
        info = MPCInfo(); model = Model()
        self._chk(self.L.srbm_get_instance_model(self.h, int(inst), C.byref(info), C.byref(model)))
        return info, model

    def close(self):
        """srbm_batch_destroy.  A batch that gait handles still borrow is NOT released by the library (return code -1): the handle is kept, so that
        it is released once the optimiser is gone, instead of leaking the device batch silently"""
        if self.h:
            for g in list(getattr(self, '_gait_handles', [])):        # optimisers created on this batch go first
                g.close()
            if self.L.srbm_batch_destroy(self.h) == 0:
                self.h = C.c_void_p()
            else:
                import warnings
                warnings.warn('srbm_batch_destroy refused: ' + self.L.srbm_last_error().decode())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError('srbm: ' + self.L.srbm_last_error().decode())

    def clone(self):
        """MPC copy constructor (mpc.cpp:1133-1181): a deep copy with its own stream and device buffers"""
        c = object.__new__(BatchMPC)
        c.L, c.cfg, c.batch, c.N, c.large, c.NUMAX, c.NSMAX = self.L, self.cfg, self.batch, self.N, self.large, self.NUMAX, self.NSMAX
        c.h = C.c_void_p()
        self._chk(self.L.srbm_batch_clone(self.h, C.byref(c.h)))
        return c

    # ---- mpc::Trajectory in and out ----
    def get_trajectory(self, first=0, count=None):
        """MPC::GetTrajectory for instances [first, first + count): a ctypes array of Trajectory records"""
        count = self.batch - first if count is None else count
        arr = (Trajectory * count)()
        self._chk(self.L.srbm_get_trajectory(self.h, int(first), int(count), arr))
        return arr

    def set_warm_start_trajectory(self, trajs, first=0):
        """MPC::SetWarmStartTrajectory (mpc.cpp:110-119); trajs: ctypes array (or list) of Trajectory records"""
        if not isinstance(trajs, C.Array):
            trajs = (Trajectory * len(trajs))(*trajs)
        self._chk(self.L.srbm_set_warm_start_trajectory(self.h, int(first), len(trajs), trajs))

    def eval_trajectory(self, time):
        """Trajectory::GetForce / GetEndEffectorLocation / GetContacts of every instance's current trajectory at time[batch]"""
        t = self._times(time)
        f = np.zeros((self.batch, 4, 3)); p = np.zeros((self.batch, 4, 3)); c = np.zeros((self.batch, 4), np.int32)
        self._chk(self.L.srbm_eval_trajectory(self.h, _d(t), _d(f), _d(p), _i(c)))
        return f, p, c

    def ee_box_center(self):
        return self._get(self.L.srbm_get_ee_box_center, self.h, np.zeros((4, 2)))

    def cost(self):
        return self._get(self.L.srbm_get_cost, self.h, np.zeros(self.batch))

    def merit(self):
        return self._get(self.L.srbm_get_merit, self.h, np.zeros(self.batch), np.zeros(self.batch))

    def add_force_cost(self, weight):
        self._chk(self.L.srbm_add_force_cost(self.h, weight))

    def avg_cost(self):
        return self._get(self.L.srbm_get_avg_cost, self.h, np.zeros(self.batch))

    def status_accumulated(self):
        """sticky accumulators over all solves since the last clear: [batch][4] = error bits, solves, not-solved, of those MaxIter"""
        return self._get(self.L.srbm_get_status_accumulated, self.h, np.zeros((self.batch, 4), np.int32))

    def clear_status_accumulators(self):
        self._chk(self.L.srbm_clear_status_accumulators(self.h))

    def executed_mfma(self):
        v = C.c_double(0)
        self._chk(self.L.srbm_get_executed_mfma(self.h, C.byref(v)))
        return v.value

    def result_record_doubles(self):
        return int(self.L.srbm_result_record_doubles(self.N))

    # ---- set-up (mpc.h:92-110) ----
    def add_quadratic_tracking_cost(self, state_des12, Q):
        a = np.ascontiguousarray(state_des12, dtype=np.float64); q = np.ascontiguousarray(Q, dtype=np.float64)
        self._chk(self.L.srbm_add_quadratic_tracking_cost(self.h, _d(a), _d(q)))

    def set_quadratic_final_cost(self, Phi):
        q = np.ascontiguousarray(Phi, dtype=np.float64)
        self._chk(self.L.srbm_set_quadratic_final_cost(self.h, _d(q)))

    def set_linear_final_cost(self, w):
        a = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.L.srbm_set_linear_final_cost(self.h, _d(a)))

    # the cost setters of instances [first, first + len(...)): one row per instance
    def add_quadratic_tracking_cost_each(self, first, state_des, Q):
        a = np.ascontiguousarray(state_des, dtype=np.float64).reshape(-1, 12)
        q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 144)
        if len(a) != len(q):
            raise ValueError('add_quadratic_tracking_cost_each: %d targets, %d weight matrices' % (len(a), len(q)))
        self._chk(self.L.srbm_add_quadratic_tracking_cost_each(self.h, int(first), len(a), _d(a), _d(q)))

    def set_quadratic_final_cost_each(self, first, Phi):
        q = np.ascontiguousarray(Phi, dtype=np.float64).reshape(-1, 144)
        self._chk(self.L.srbm_set_quadratic_final_cost_each(self.h, int(first), len(q), _d(q)))

    def set_linear_final_cost_each(self, first, w):
        a = np.ascontiguousarray(w, dtype=np.float64).reshape(-1, 12)
        self._chk(self.L.srbm_set_linear_final_cost_each(self.h, int(first), len(a), _d(a)))

    def add_force_cost_each(self, first, weight):
        a = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        self._chk(self.L.srbm_add_force_cost_each(self.h, int(first), len(a), _d(a)))

    def set_solver_step_rule(self, tol_step, start_mu=0.0):
        self._chk(self.L.srbm_set_solver_step_rule(self.h, tol_step, start_mu))

    def enable_fast_termination(self, start_mu=FAST_START_MU):
        """opt into the step rule (and, for srbm_rti_advance, the lower-start attempt) at the values the bench line is taken with"""
        self.set_solver_step_rule(FAST_TOL_STEP, start_mu)

    def enable_lower_start(self, start_mu=FAST_START_MU):
        """the lower starting point alone: every solve still ends by the reference's gap criterion (tol_step 0), srbm_rti_advance first attempts it
        from the linearisation point"""
        self.set_solver_step_rule(0.0, start_mu)

    def solve_flags(self):
        """per instance, of the LAST solve: bit 0 ended through the step rule, bit 1 began with a lower-start attempt, bit 2 the attempt was repeated"""
        return self._get(self.L.srbm_get_solve_flags, self.h, np.zeros(self.batch, np.int32))

    def solver_step_rule(self):
        a = C.c_double(0); b = C.c_double(0)
        self._chk(self.L.srbm_get_solver_step_rule(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def solver_counters(self):
        c = (C.c_longlong * 4)()
        self._chk(self.L.srbm_get_solver_counters(self.h, c))
        return dict(solves=c[0], step_rule=c[1], low_tried=c[2], low_failed=c[3])

    def set_state_trajectory_warm_start(self, states):
        a = self._bcast(states, 13)
        self._chk(self.L.srbm_set_state_trajectory_warm_start(self.h, _d(a)))

    def set_solver_tolerances(self, gap_abs, gap_rel, feas, max_iter=200):
        self._chk(self.L.srbm_set_solver_tolerances(self.h, gap_abs, gap_rel, feas, int(max_iter)))

    def _times(self, time):             # a time, or one per instance, as time[batch]
        return np.ascontiguousarray(np.broadcast_to(np.asarray(time, dtype=np.float64), (self.batch,)))

    def _get(self, fn, h, *outs, tail=()):
        """the read-back getters: fn(h, *outs, *tail) on the caller's zeroed arrays (each passed as a pointer of its dtype), check, return them"""
        self._chk(fn(h, *[(_i if a.dtype == np.int32 else _d)(a) for a in outs], *tail))
        return outs[0] if len(outs) == 1 else outs

    # leading dimensions of the result records with the capacities of the loaded build (include/srbm_rti.h: NX, NM of srbm_pack_results_dev)
    _ld_primal = property(lambda self: (self.N + 1) * 12 + self.NUMAX)
    _ld_dual = property(lambda self: (self.N + 1) * 12 + 6 * self.NSMAX + 16 * (self.N - 3) + 16)

    def _bcast(self, a, width):
        a = np.asarray(a, dtype=np.float64)
        if a.size == width:
            a = np.tile(a.reshape(1, width), (self.batch, 1))
        return np.ascontiguousarray(a.reshape(self.batch, width))

    # ---- solves ----
    def create_initial_run(self, state, ee):
        s = self._bcast(state, 13); e = self._bcast(ee, 12)
        self._chk(self.L.srbm_create_initial_run(self.h, _d(s), _d(e)))

    def get_real_time_update(self, state, init_time, ee):
        s = self._bcast(state, 13); e = self._bcast(ee, 12)
        t = self._times(init_time)
        self._chk(self.L.srbm_get_real_time_update(self.h, _d(s), _d(t), _d(e)))

    def get_real_time_update_dev(self, state_ptr, time_ptr, ee_ptr):
        self._chk(self.L.srbm_get_real_time_update_dev(self.h, state_ptr, time_ptr, ee_ptr))

    def rti_advance(self, first_index, steps):
        self._chk(self.L.srbm_rti_advance(self.h, int(first_index), int(steps)))

    def rti_advance_unfused(self, first_index, steps):
        self._chk(self.L.srbm_rti_advance_unfused(self.h, int(first_index), int(steps)))

    # ---- closed-loop rollout harness (include/srbm_rti.h: srbm_plant_*, srbm_closed_loop_advance; the MPC period: mpc_period.py) ----
    def plant_set_state(self, state):
        self._chk(self.L.srbm_plant_set_state(self.h, _d(self._bcast(state, 13))))

    def plant_state(self):
        return self._get(self.L.srbm_plant_get_state, self.h, np.zeros((self.batch, 13)))

    def plant_set_push(self, time=None, impulse=None):
        """one push per instance: lin-mom += impulse[:3], ang-mom += impulse[3:] when the plant passes `time`; None clears"""
        if time is None:
            self._chk(self.L.srbm_plant_set_push(self.h, None, None))
        else:
            self._chk(self.L.srbm_plant_set_push(self.h, _d(self._bcast(time, 1)), _d(self._bcast(impulse, 6))))

    def closed_loop_advance(self, first_index, steps, substeps=1, advance_time=False):
        """iterations first_index .. first_index + steps - 1: iteration i of instance b integrates its plant from i p over p, p its MPC period
        (mpc_period.plant_set_period; the node step dt where none is set), and solves at i p + p; asynchronous"""
        self._chk(self.L.srbm_closed_loop_advance(self.h, int(first_index), int(steps), int(substeps), int(bool(advance_time))))

    # ---- the step log: every step of a multi-step launch (include/srbm_rti.h: srbm_step_log_*) ----
    def step_log_enable(self, max_steps):
        """room for max_steps steps of this batch, cursor 0; 0 disables logging and frees the buffer.  A clone has logging off"""
        self._chk(self.L.srbm_step_log_enable(self.h, int(max_steps)))

    def step_log_reset(self):
        self._chk(self.L.srbm_step_log_reset(self.h))

    def step_log_count(self):
        n = C.c_int(0)
        self._chk(self.L.srbm_step_log_count(self.h, C.byref(n)))
        return n.value

    def step_log(self, first=0, count=None):
        """the records of slots [first, first + count) as an array [count][batch][STEP_LOG_DOUBLES] (STEP_LOG_FIELDS names the columns); synchronous"""
        count = self.step_log_count() - first if count is None else count
        a = np.zeros((max(int(count), 0), self.batch, STEP_LOG_DOUBLES))
        self._chk(self.L.srbm_step_log_get(self.h, int(first), int(count), _d(a)))
        return a

    def step_log_copy_dev(self, ptr, first=0, count=None):
        """the same records to device memory at `ptr`, on the batch's stream, without synchronisation"""
        count = self.step_log_count() - first if count is None else count
        self._chk(self.L.srbm_step_log_copy_dev(self.h, int(first), int(count), ptr))

    def synchronize(self):
        self._chk(self.L.srbm_synchronize(self.h))

    def stream(self):
        return self.L.srbm_stream(self.h)

    def update_contact_times(self, times):
        a = np.ascontiguousarray(times, dtype=np.float64)
        assert a.ndim == 3 and a.shape[0] == self.batch and a.shape[1] == 4
        self._chk(self.L.srbm_update_contact_times(self.h, _d(a), a.shape[2]))

    def adjust_for_current_contacts(self, time, in_contact):
        t = self._times(time)
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(in_contact, dtype=np.int32), (self.batch, 4)))
        self._chk(self.L.srbm_adjust_for_current_contacts(self.h, _d(t), _i(c)))

    # ---- trajectory -> whole-body targets ----
    def forward_kinematics(self, q):
        """SingleRigidBodyModel::GetEndEffectorLocations: q[batch][19] -> [batch][4][3]"""
        qq = self._bcast(q, 19); ee = np.zeros((self.batch, 4, 3))
        self._chk(self.L.srbm_forward_kinematics(self.h, _d(qq), _d(ee)))
        return ee

    def inverse_kinematics(self, state, ee, q_guess):
        """SingleRigidBodyModel::InverseKinematics for every instance -> (q [batch][19], iterations [batch][4], status [batch])"""
        s = self._bcast(state, 13); e = self._bcast(ee, 12); g = self._bcast(q_guess, 19)
        q = np.zeros((self.batch, 19)); it = np.zeros((self.batch, 4), np.int32); st = np.zeros(self.batch, np.int32)
        self._chk(self.L.srbm_inverse_kinematics(self.h, _d(s), _d(e), _d(g), _d(q), _i(it), _i(st)))
        return q, it, st

    def get_targets_from_traj_dev(self, time_ptr, q_des_ptr, v_des_ptr, force_des_ptr, status_ptr):
        """the same on device pointers (ints, e.g. torch tensors' data_ptr()): one launch on the batch's stream, no copy, no synchronisation"""
        self._chk(self.L.srbm_get_targets_from_traj_dev(self.h, time_ptr, q_des_ptr, v_des_ptr, force_des_ptr, status_ptr))

    def eval_trajectory_dev(self, time_ptr, force_ptr, pos_ptr, in_contact_ptr):
        """Trajectory::GetForce / GetEndEffectorLocation / contact flags on device pointers (one launch, no copy)"""
        self._chk(self.L.srbm_eval_trajectory_dev(self.h, time_ptr, force_ptr, pos_ptr, in_contact_ptr))

    def qp_control_dev(self, q, v, contact, q_des, v_des, force_des, control, qp_sol, status):
        self._chk(self.L.srbm_qp_control_dev(self.h, q, v, contact, q_des, v_des, force_des, control, qp_sol, status))

    def get_targets_from_traj(self, time, q_des):
        """MPCController::GetTargetsFromTraj on the current trajectories -> (q_des, v_des [batch][18], force_des [batch][4][3], status)"""
        t = self._times(time)
        q = self._bcast(q_des, 19).copy(); v = np.zeros((self.batch, 18)); f = np.zeros((self.batch, 4, 3)); st = np.zeros(self.batch, np.int32)
        self._chk(self.L.srbm_get_targets_from_traj(self.h, _d(t), _d(q), _d(v), _d(f), _i(st)))
        return q, v, f, st

    def qp_control(self, q, v, contact, q_des, v_des, force_des, dump=False):
        """QPControl::ComputeControlAction for every instance -> (control [batch][36], qp_sol [batch][30], status, iterations[, QP dump])"""
        B = self.batch
        qq = self._bcast(q, 19); vv = self._bcast(v, 18); qd = self._bcast(q_des, 19); vd = self._bcast(v_des, 18); fd = self._bcast(force_des, 12)
        con = np.ascontiguousarray(np.broadcast_to(np.asarray(contact, dtype=np.int32), (B, 4)))
        ctl = np.zeros((B, 36)); sol = np.zeros((B, 30)); st = np.zeros(B, np.int32)
        dmp = np.zeros((B, 50 * 30 + 100 + 60)) if dump else None
        self._chk(self.L.srbm_qp_control(self.h, _d(qq), _d(vv), _i(con), _d(qd), _d(vd), _d(fd), _d(ctl), _d(sol), _i(st), _d(dmp) if dump else None))
        out = (ctl, sol, st & 255, st >> 8)
        if dump:
            A = dmp[:, :1500].reshape(B, 50, 30)
            out += (dict(A=A, lb=dmp[:, 1500:1550], ub=dmp[:, 1550:1600], P=dmp[:, 1600:1630], w=dmp[:, 1630:1660]),)
        return out

    # ---- the reference's statistics log ----
    def print_stat_header(self, fh):
        """header block of MPC::PrintStatLineToFile (mpc.cpp:901-939), same field widths.  (std::left is set on the stream while
        the header is written and stays set: every column of the table is LEFT aligned in its 15 characters.)"""
        cw, tw = 15, 150
        c = self.cfg
        import time as _time
        fh.write('-' * tw + '\n' + ' ' * (tw // 2 - 7) + 'MPC Statistics\n')
        fh.write('MPC started at: ' + _time.ctime() + '\n')                     # std::ctime of the wall clock (mpc.cpp:910-915)
        fh.write('Number of nodes: %d\nMPC time step: %g\nForce bounds: %g\nEnd Effector box size: %g %g\n' %
                 (self.N, c['integrator_dt'], c['force_bound'], c['ee_box_size'][0], c['ee_box_size'][1]))
        fh.write('Force cost: %g\nFoot offset: %g\nSwing height: %g\n' % (c['force_cost'], c['foot_offset'], c['swing_height']))
        fh.write('-' * tw + '\n')
        cols = ['Solve #', 'Time (ms)', 'Constraints', 'Step Norm', 'Alpha', 'Cost', 'Merit', 'Merit dd', 'Solve Type', 'QP Cost']
        fh.write(''.join(n.ljust(cw) for n in cols) + '\n' + '-' * tw + '\n')

    def print_stat_line(self, fh, solve_number, time_ms, inst=0):
        """one table row of MPC::PrintStatLineToFile (mpc.cpp:974-989) for instance `inst` from the last solve.  Merit =
        cost + mu * L1 dynamics defect (mpc.cpp:749-757, mu = 5000), Merit dd = its directional derivative along the step."""
        st, err = self.status()
        merit, merit_dd = self.merit()
        fh.write(format_stat_line(solve_number, time_ms, self.stats()[inst], merit[inst], merit_dd[inst], st[inst]))

    # ---- measurement aids ----
    def enable_kernel_timing(self, max_launches):
        self._chk(self.L.srbm_enable_kernel_timing(self.h, int(max_launches)))

    def kernel_timing(self):
        ms = C.c_double(0); n = C.c_int(0)
        self._chk(self.L.srbm_get_kernel_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_timings(self, max_launches=64):
        ms = np.zeros(max_launches); n = C.c_int(0)
        self._chk(self.L.srbm_get_kernel_timings(self.h, _d(ms), int(max_launches), C.byref(n)))
        return ms[:min(n.value, max_launches)].copy()

    def debug_launch_info(self):
        """srbm_debug_get_launch_info: the kernel the last srbm_rti_advance / srbm_closed_loop_advance with steps > 0 took (host-side record, no sync)"""
        a = (C.c_int * 4)()
        self._chk(self.L.srbm_debug_get_launch_info(self.h, a))
        return dict(n_cu=a[0], kernel=(None, 'srbm_rti_fused', 'srbm_rti_fused_long', 'srbm_rti_queued', 'srbm_rti_queued_long')[a[1]], steps=a[2], queued=bool(a[3]))

    def work_counters(self):
        it = C.c_double(0); fl = C.c_double(0)
        self._chk(self.L.srbm_get_work_counters(self.h, C.byref(it), C.byref(fl)))
        return it.value, fl.value

    def pack_results_dev(self, ptr, ld):
        self._chk(self.L.srbm_pack_results_dev(self.h, ptr, int(ld)))

    # ---- multi-GPU: RCCL all-gather of the result records through the C-ABI (include/srbm_rti.h: srbm_allgather_results) ----
    def rccl_unique_id(self):
        """ncclGetUniqueId (one rank calls it, the 128 bytes travel to the others by the host's own rendezvous)"""
        buf = (C.c_ubyte * RCCL_UNIQUE_ID_BYTES)()
        self._chk(self.L.srbm_rccl_get_unique_id(buf))
        return bytes(buf)

    def rccl_comm_init_rank(self, world, rank, id_bytes):
        """ncclCommInitRank on the batch's device; returns the ncclComm_t as an integer handle"""
        assert len(id_bytes) == RCCL_UNIQUE_ID_BYTES
        comm = C.c_void_p(0)
        buf = (C.c_ubyte * RCCL_UNIQUE_ID_BYTES).from_buffer_copy(id_bytes)
        self._chk(self.L.srbm_rccl_comm_init_rank(self.h, int(world), int(rank), buf, C.byref(comm)))
        return comm.value

    def rccl_comm_destroy(self, comm):
        self._chk(self.L.srbm_rccl_comm_destroy(comm))

    def allgather_results(self, comm, out_ptr):
        """this rank's result records packed into their slot of out[world * batch][record_doubles] (device pointer) and ONE in-place ncclAllGather
        on the batch's stream; asynchronous (synchronize() before reading)"""
        self._chk(self.L.srbm_allgather_results(self.h, comm, out_ptr))

    def pack_results(self):
        """the result records of srbm_pack_results_dev in a host array [batch][srbm_result_record_doubles(N)]"""
        ld = self.result_record_doubles()
        return self._get(self.L.srbm_pack_results, self.h, np.zeros((self.batch, ld)), tail=(ld,))

    # ---- results ----
    def sizes(self):
        return self._get(self.L.srbm_get_sizes, self.h, np.zeros((self.batch, 8), np.int32))

    def status(self):
        return self._get(self.L.srbm_get_status, self.h, np.zeros(self.batch, np.int32), np.zeros(self.batch, np.int32))

    def stats(self):
        return self._get(self.L.srbm_get_stats, self.h, np.zeros((self.batch, 8)))

    def qp_cost(self):
        return self._get(self.L.srbm_get_qp_cost, self.h, np.zeros(self.batch))

    def qp_solution(self):
        return self._get(self.L.srbm_get_qp_solution, self.h, np.zeros((self.batch, self._ld_primal)), tail=(self._ld_primal,))

    def raw_qp_minimiser(self):
        return self._get(self.L.srbm_get_raw_qp_minimiser, self.h, np.zeros((self.batch, self._ld_primal)), tail=(self._ld_primal,))

    def dual_solution(self):
        ld = self._ld_dual
        return self._get(self.L.srbm_get_dual_solution, self.h, np.zeros((self.batch, ld)), np.zeros((self.batch, ld)), tail=(ld,))

    def trajectory_states(self):
        return self._get(self.L.srbm_get_trajectory_states, self.h, np.zeros((self.batch, self.N + 1, 13)))

    def knots(self, inst):
        t = np.zeros((4, 32)); kd = np.zeros((4, 32), np.int32); nk = np.zeros(4, np.int32)
        fv = np.zeros((4, 3, 32, 2)); pv = np.zeros((4, 2, 32)); box = np.zeros(2)
        self._chk(self.L.srbm_get_knots(self.h, int(inst), _d(t), _i(kd), _i(nk), _d(fv), _d(pv), _d(box)))
        return dict(times=t, kinds=kd, nk=nk, fvals=fv, pvals=pv, box=box)

    def export_qp(self, inst):
        sz = self.sizes()[inst]
        n, m = int(sz[0]), int(sz[1])
        A = np.zeros((m, n)); b = np.zeros(m); P = np.zeros((n, n)); q = np.zeros(n)
        self._chk(self.L.srbm_export_qp(self.h, int(inst), _d(A), _d(b), _d(P), _d(q)))
        return A, b, P, q

    def param_partials(self, inst, ee, idx):
        """MPCSingleRigidBody::ComputeParamPartialsClarabel (mpc_single_rigid_body.cpp:642-792) as dense matrices: (dA, dG, db, dh) of the QP
        of the last solve w.r.t. contact time `idx` of foot `ee`, evaluated on the current trajectory of instance `inst`."""
        sz = self.sizes()[inst]
        n, me, mi = int(sz[0]), int(sz[2]), int(sz[3])
        dA = np.zeros((me, n)); dG = np.zeros((mi, n)); db = np.zeros(me); dh = np.zeros(mi)
        self._chk(self.L.srbm_gait_get_param_partials(self.h, int(inst), int(ee), int(idx), _d(dA), _d(dG), _d(db), _d(dh)))
        return dA, dG, db, dh


class BatchGaitOptimizer:
    """mpc::GaitOptimizer (/root/reference/mpc/include/gait_optimizer.h) for every instance of a BatchMPC: same method
    names in snake_case, contact-time vectors as [batch][32] rows (foot after foot, `counts` entries per foot)."""
    NV = 32
    LS_SIZE = 10

    def __init__(self, mpc):
        self.mpc = mpc
        self.L = mpc.L
        self.g = C.c_void_p()
        mpc._chk(self.L.srbm_gait_create(mpc.h, C.byref(self.g)))
        import weakref
        if not hasattr(mpc, '_gait_handles'):
            mpc._gait_handles = weakref.WeakSet()
        mpc._gait_handles.add(self)          # BatchMPC.close() releases the optimisers that borrow it first

    def close(self):
        if self.g:
            self.L.srbm_gait_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_contact_times_from_trajectory(self):
        self.mpc._chk(self.L.srbm_gait_set_contact_times_from_trajectory(self.g))

    def contact_times(self):
        return self.mpc._get(self.L.srbm_gait_get_contact_times, self.g, np.zeros((self.mpc.batch, self.NV)), np.zeros((self.mpc.batch, 4), np.int32))

    def compute_sensitivity(self):
        self.mpc._chk(self.L.srbm_gait_compute_sensitivity(self.g))

    def sensitivity(self):
        m = self.mpc
        ld = m._ld_primal + m._ld_dual           # [dz; dlam; dnu]: one entry per primal and per dual variable
        return m._get(self.L.srbm_gait_get_sensitivity, self.g, np.zeros((m.batch, ld)), tail=(ld,))

    def compute_gradient(self):
        self.mpc._chk(self.L.srbm_gait_compute_gradient(self.g))

    def gradient(self):
        m = self.mpc
        return m._get(self.L.srbm_gait_get_gradient, self.g, np.zeros((m.batch, self.NV)), np.zeros(m.batch, np.int32))

    def set_gradient(self, dHdth, valid=1):
        """a gradient supplied by the caller: dHdth[batch][<= 32] (or one row for every instance), valid[batch] (or one value)"""
        a = np.zeros((self.mpc.batch, self.NV))
        gr = np.asarray(dHdth, dtype=np.float64)
        a[:, :gr.shape[-1]] = gr
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(valid, dtype=np.int32), (self.mpc.batch,)))
        self.mpc._chk(self.L.srbm_gait_set_gradient(self.g, _d(a), _i(v)))

    def optimize_contact_times(self, time):
        m = self.mpc
        t = m._times(time)
        m._chk(self.L.srbm_gait_optimize_contact_times(self.g, _d(t)))

    def lp_result(self):
        m = self.mpc
        return m._get(self.L.srbm_gait_get_lp_result, self.g, np.zeros(m.batch, np.int32), np.zeros(m.batch))

    def rti_advance(self, first_run_num, steps, gait_opt_freq):
        self.mpc._chk(self.L.srbm_gait_rti_advance(self.g, int(first_run_num), int(steps), int(gait_opt_freq)))

    def set_step(self, step):
        a = np.zeros((self.mpc.batch, self.NV))
        st = np.asarray(step, dtype=np.float64)
        a[:, :st.shape[-1]] = st
        self.mpc._chk(self.L.srbm_gait_set_step(self.g, _d(a)))

    def step(self):
        return self.mpc._get(self.L.srbm_gait_get_step, self.g, np.zeros((self.mpc.batch, self.NV)))

    def line_search(self, state, init_time, ee):
        m = self.mpc
        s = m._bcast(state, 13); e = m._bcast(ee, 12)
        t = m._times(init_time)
        imin = np.zeros(m.batch, np.int32); costs = np.zeros((m.batch, self.LS_SIZE))
        m._chk(self.L.srbm_gait_line_search(self.g, _d(s), _d(t), _d(e), _i(imin), _d(costs)))
        return imin, costs

    def candidates(self):
        """the candidate batch of the last line search as a BORROWED BatchMPC view (read-back entries only): candidate c of instance b at b * 10 + c"""
        v = object.__new__(BatchMPC)
        m = self.mpc
        v.N, v.large, v.L, v.NUMAX, v.NSMAX, v.cfg = m.N, m.large, m.L, m.NUMAX, m.NSMAX, m.cfg
        v.batch = m.batch * self.LS_SIZE
        v.h = C.c_void_p(self.L.srbm_gait_debug_candidates(self.g))
        v.close = lambda: None                      # not ours to destroy
        return v

    def candidate_status(self):
        n = self.mpc.batch * self.LS_SIZE
        st, err = self.mpc._get(self.L.srbm_gait_get_candidate_status, self.g, np.zeros(n, np.int32), np.zeros(n, np.int32))
        return st.reshape(-1, self.LS_SIZE), err.reshape(-1, self.LS_SIZE)


def dense_row_placement(N, nu, wc, large=False):
    """srbm_debug_dense_row_placement (host only, no GPU): where the IPM of that build puts the 2 (N - 3) compact dense state rows of width wc
    at n_u = nu -- (rows in the tail of the packed-matrix window, rows behind the LDS map, True if all are in LDS; False: read from L2)"""
    L = lib(large)
    out = (C.c_int * 3)()
    if L.srbm_debug_dense_row_placement(int(N), int(nu), int(wc), out) != 0:
        raise ValueError(L.srbm_last_error().decode())
    return out[0], out[1], bool(out[2])


def condensed(mpc, inst):
    """srbm_debug_get_condensed: what the condensing kernel left in the work record of instance `inst` at its last solve, trimmed to the
    instance's sizes -- H (n_u x n_u, both triangles filled from the packed lower one), g [n_u], the compact dense state rows Sig
    [2 (N - 3)][n_u] (row 2 (k - 4) + c: position c of node k on the force variables of coordinate c), sig0 [2 (N - 3)], n_u, the error bits;
    `packed` is the packed lower triangle as the kernel wrote it (what scripts/dev_bitwise_ab.py compares byte for byte)"""
    NU, rows_cap, rows = mpc.NUMAX, 2 * (mpc.L.capacity['N'] - 3), 2 * (mpc.N - 3)
    Hp = np.zeros(NU * (NU + 1) // 2); g = np.zeros(NU); Sig = np.zeros((rows_cap, NU)); sig0 = np.zeros(rows_cap)
    nu = np.zeros(1, np.int32); err = np.zeros(1, np.int32)
    read = mpc.L.srbm_debug_get_condensed
    mpc._chk(read(mpc.h, int(inst), _d(Hp), _d(g), _d(Sig), _d(sig0), _i(nu), _i(err)))
    n = int(nu[0])
    H = np.zeros((n, n))
    H[np.tril_indices(n)] = Hp[:n * (n + 1) // 2]
    H = H + np.tril(H, -1).T
    return dict(H=H, g=g[:n].copy(), Sig=Sig[:rows, :n].copy(), sig0=sig0[:rows].copy(), nu=n, err=int(err[0]), packed=Hp[:n * (n + 1) // 2].copy())
