"""The C++ host side above the C-ABI (tests/cpp/cabi_batch_smoke.cpp drives include/srbm_rti.h from C++ for a batch; include/mpc_facade: the reference's
class and method names).  CPU: the header and the smoke program compile with g++ and link against libsrbm_rti.so.
GPU: the program's read-backs equal the ctypes path (same library, same call sequence: bit-identical)."""
import json
import os
import subprocess

import numpy as np
import pytest

from srbm_loader import host
from srbm_loader.workloads import EE_NOMINAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# <Eigen/Core> for the facade headers: the system's if there is one, else the stand-in of the tests (this container has no Eigen)
EIGEN_INC = next((d for d in ('/usr/include/eigen3', '/usr/local/include/eigen3') if os.path.exists(os.path.join(d, 'Eigen', 'Core'))),
                 os.path.join(ROOT, 'tests', 'cpp', 'eigen_standin'))
CPP = os.path.join(ROOT, 'tests', 'cpp')
# the reference's robot description (xacro output), stored as a data fixture: the facade's URDF reader has to merge its fixed links itself
A1_URDF = os.path.join(ROOT, 'tests', 'golden', 'a1.urdf')


def write_cfg_inc(cfg, path):
    tgt = np.array(cfg['srb_target'], float)
    tt = host.manifold_to_tangent(tgt)
    arr = lambda name, v: 'static const double %s[%d] = {%s};\n' % (name, len(v), ', '.join(repr(float(x)) for x in v))
    with open(path, 'w') as f:
        f.write('static const int kNumNodes = %d;\n' % cfg['num_nodes'])
        for name, key in [('kDt', 'integrator_dt'), ('kMu', 'friction_coef'), ('kForceBound', 'force_bound'), ('kSwing', 'swing_height'),
                          ('kFootOffset', 'foot_offset'), ('kForceCost', 'force_cost'), ('kMass', 'mass')]:
            f.write('static const double %s = %r;\n' % (name, float(cfg[key])))
        f.write(arr('kBox', cfg['ee_box_size'])); f.write(arr('kIr', np.array(cfg['Ir']).reshape(-1)))
        f.write(arr('kHip', np.array(cfg['hip_xy']).reshape(-1))); f.write(arr('kQdiag', cfg['Q_srbd_diag']))
        f.write(arr('kInit', cfg['srb_init'])); f.write(arr('kTarget13', tgt)); f.write(arr('kTargetTangent', tt))
        gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'a1_constants_a1_configuration.json')))
        f.write(arr('kInitConfig', gold['source']['init_config']))
        # whole-body controller gains (row f3; tests/cpp/wbc_driver.cpp)
        for name, key in [('kTorqueBounds', 'torque_bounds'), ('kKpJoint', 'kp_joint_gains'), ('kKdJoint', 'kd_joint_gains'), ('kBasePosGains', 'base_pos_gains'),
                          ('kBaseAngGains', 'base_ang_gains')]:
            f.write(arr(name, cfg[key]))
        for name, key in [('kLegWeight', 'leg_tracking_weight'), ('kTorsoWeight', 'torso_tracking_weight'), ('kForceWeight', 'force_tracking_weight')]:
            f.write('static const double %s = %r;\n' % (name, float(cfg[key])))


def build_program(tmpdir):
    cfg = host.load_config('a1_configuration')
    host.build()
    write_cfg_inc(cfg, os.path.join(tmpdir, 'cfg.inc'))
    exe = os.path.join(tmpdir, 'facade_smoke')
    libdir = os.path.dirname(host.LIB_PATH)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-I', EIGEN_INC, '-I', tmpdir,
                           os.path.join(CPP, 'cabi_batch_smoke.cpp'), '-o', exe, '-L', libdir, '-lsrbm_rti', '-Wl,-rpath,' + libdir])
    return cfg, exe


def test_cpp_host_side_compiles_and_links(tmp_path):
    cfg, exe = build_program(str(tmp_path))
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_host_side_equals_ctypes_path(tmp_path):
    cfg, exe = build_program(str(tmp_path))
    out = subprocess.check_output([exe], text=True)
    lines = out.strip().splitlines()
    head = lines[0].split()
    vals = {}
    for ln in lines[1:]:
        k, i, v = ln.split()
        vals.setdefault(k, []).append(float(v))
    # the same sequence through ctypes
    s0 = np.array(cfg['srb_init'], float)
    ee0 = EE_NOMINAL
    g = host.BatchMPC.cold_start(cfg, [s0] * 2, ee0, initial_run=False)
    assert g.solver_step_rule() == (0.0, 0.0)
    g.create_initial_run(s0, ee0)
    g.rti_advance(0, 4); g.synchronize()
    gait = host.BatchGaitOptimizer(g)
    gait.compute_gradient()
    grad, valid = gait.gradient()
    t = 4 * cfg['integrator_dt']
    gait.optimize_contact_times(t)
    step = gait.step()
    st1 = g.trajectory_states()[:, 1, :]
    imin, costs = gait.line_search(st1, t, ee0)
    st, err = g.status()
    sz = g.sizes()
    x = g.qp_solution()
    assert [int(v) for v in head[1:3]] == [int(st[0]), int(st[1])]
    assert int(head[7]) == sz[0, 0] and int(head[9]) == sz[0, 1] and int(head[11]) == valid[0] and int(head[13]) == imin[0]
    assert np.array_equal(np.array(vals['grad']), grad[0, :20])
    assert np.array_equal(np.array(vals['step']), step[0, :20])
    assert np.array_equal(np.array(vals['x']), x[0, :40])


# ---------------- the collective on the C side of the boundary (include/srbm_rti.h: srbm_allgather_results) ----------------
def build_allgather_program(tmpdir):
    cfg = host.load_config('a1_configuration')
    host.build()
    write_cfg_inc(cfg, os.path.join(tmpdir, 'cfg.inc'))
    exe = os.path.join(tmpdir, 'cabi_allgather_smoke')
    libdir = os.path.dirname(host.LIB_PATH)
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__', '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(rocm, 'include'),
                           '-I', tmpdir, os.path.join(CPP, 'cabi_allgather_smoke.cpp'), '-o', exe, '-L', libdir, '-lsrbm_rti', '-L', os.path.join(rocm, 'lib'), '-lrccl',
                           '-lamdhip64', '-Wl,-rpath,' + libdir, '-Wl,-rpath,' + os.path.join(rocm, 'lib')])
    return cfg, exe


def test_cpp_allgather_host_compiles_and_links(tmp_path):
    """a C++ host that links RCCL itself and passes its own ncclComm_t across the C-ABI; the library itself must NOT depend on
    RCCL at link time (it binds the process's copy at run time)"""
    cfg, exe = build_allgather_program(str(tmp_path))
    assert os.path.exists(exe)
    needed = subprocess.check_output(['readelf', '-d', host.LIB_PATH], text=True)
    assert 'librccl' not in needed


@pytest.mark.gpu
def test_cpp_allgather_of_one_rank_equals_the_packed_records(tmp_path):
    """world size 1 on the one-GPU box: srbm_allgather_results (in-place ncclAllGather on the batch's stream) with the HOST's communicator and with
    one from srbm_rccl_comm_init_rank both reproduce srbm_pack_results bit for bit"""
    cfg, exe = build_allgather_program(str(tmp_path))
    vals = parse_dump(subprocess.check_output([exe], text=True, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))))
    g = host.BatchMPC(cfg, 1)
    assert vals['record_doubles'] == [float(g.result_record_doubles())]
    assert vals['own_comm_equal'] == [1.0] and vals['helper_comm_equal'] == [1.0]
    assert all(v <= 1.0 for v in vals['status']) and len(set(vals['x0'])) == 3


# ---------------- include/mpc_facade/mpc.h: the reference's own class names and signatures ----------------
def build_callsites(tmpdir):
    cfg = host.load_config('a1_configuration')
    host.build()
    write_cfg_inc(cfg, os.path.join(tmpdir, 'cfg.inc'))
    exe = os.path.join(tmpdir, 'controller_driver')
    libdir = os.path.dirname(host.LIB_PATH)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-I', EIGEN_INC, '-I', tmpdir,
                           os.path.join(CPP, 'controller_driver.cpp'), '-o', exe, '-L', libdir, '-lsrbm_rti', '-Wl,-rpath,' + libdir])
    return cfg, exe


def write_urdf_from_golden(path):
    """A URDF with the structure the library is built for -- floating base, trunk, four legs of (hip x, thigh y, calf y) revolute joints and a
    fixed foot frame -- written from the committed constants tests/golden/a1_constants_a1_configuration.json (leg joint origins, the thirteen
    bodies with fixed links already merged).  It is DATA for the facade's URDF reader: reading it back must reproduce those constants."""
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'a1_constants_a1_configuration.json')))
    v3 = lambda v: ' '.join(repr(float(x)) for x in v)
    def link(name, body):
        if body is None:
            return '  <link name="%s"/>\n' % name
        I = np.array(body['inertia'])
        return ('  <link name="%s">\n    <inertial>\n      <origin rpy="0 0 0" xyz="%s"/>\n      <mass value="%r"/>\n'
                '      <inertia ixx="%r" ixy="%r" ixz="%r" iyy="%r" iyz="%r" izz="%r"/>\n    </inertial>\n  </link>\n' %
                (name, v3(body['com']), float(body['mass']), float(I[0, 0]), float(I[0, 1]), float(I[0, 2]), float(I[1, 1]), float(I[1, 2]), float(I[2, 2])))
    def joint(name, typ, parent, child, xyz, axis=None):
        ax = '    <axis xyz="%s"/>\n' % v3(axis) if axis is not None else ''
        return '  <joint name="%s" type="%s">\n    <origin rpy="0 0 0" xyz="%s"/>\n    <parent link="%s"/>\n    <child link="%s"/>\n%s  </joint>\n' % (name, typ, v3(xyz), parent, child, ax)
    out = '<?xml version="1.0"?>\n<robot name="quadruped_from_constants">\n' + link('base', None) + joint('floating_base', 'fixed', 'base', 'trunk', [0, 0, 0]) + link('trunk', gold['body_model'][0])
    for e, leg in enumerate(('FL', 'FR', 'RL', 'RR')):
        o = gold['leg_origins'][leg]
        out += joint(leg + '_hip_joint', 'revolute', 'trunk', leg + '_hip', o[0], [1, 0, 0]) + link(leg + '_hip', gold['body_model'][1 + 3 * e])
        out += joint(leg + '_thigh_joint', 'revolute', leg + '_hip', leg + '_thigh', o[1], [0, 1, 0]) + link(leg + '_thigh', gold['body_model'][2 + 3 * e])
        out += joint(leg + '_calf_joint', 'revolute', leg + '_thigh', leg + '_calf', o[2], [0, 1, 0]) + link(leg + '_calf', gold['body_model'][3 + 3 * e])
        out += joint(leg + '_foot_fixed', 'fixed', leg + '_calf', leg + '_foot', o[3]) + link(leg + '_foot', None)
    out += '</robot>\n'
    open(path, 'w').write(out)
    return gold


def build_wbc_callsites(tmpdir):
    cfg = host.load_config('a1_configuration')
    host.build()
    write_cfg_inc(cfg, os.path.join(tmpdir, 'cfg.inc'))
    exe = os.path.join(tmpdir, 'wbc_driver')
    libdir = os.path.dirname(host.LIB_PATH)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-I', EIGEN_INC, '-I', tmpdir,
                           os.path.join(CPP, 'wbc_driver.cpp'), '-o', exe, '-L', libdir, '-lsrbm_rti', '-Wl,-rpath,' + libdir])
    return cfg, exe


def parse_dump(out):
    vals = {}
    for ln in out.strip().splitlines():
        parts = ln.split()
        if len(parts) == 3:
            try:
                vals.setdefault(parts[0], []).append(float(parts[2]))
            except ValueError:
                pass
    return vals


def test_controller_driver_compiles_against_the_mpc_facade(tmp_path):
    """the builder-written behaviour driver (tests/cpp/controller_driver.cpp: MPCController::MPCUpdate and
    MPCController::GaitOpt, controllers/mpc_controller.cpp:286-399, :518-566, the same methods in the same order, the MPC, the gait optimiser and the
    trajectory held BY VALUE) compiles warning-free against include/mpc_facade/mpc.h and links against the C-ABI library."""
    cfg, exe = build_callsites(str(tmp_path))
    assert os.path.exists(exe)


def test_facade_urdf_reader_reproduces_the_model_constants(tmp_path):
    """MPC(const MPCInfo&, const std::string& robot_urdf) gets mass, Ir and the hip origins from the URDF as the reference does
    through pinocchio (mpc/models/model.cpp:27, single_rigid_body_model.cpp:33-37,258-308).  Reads the reference's URDF
    asset (tests/golden/a1.urdf), against the committed fixture of oracle/tools/a1_constants.py."""
    cfg, exe = build_callsites(str(tmp_path))
    vals = parse_dump(subprocess.check_output([exe, A1_URDF, '0'], text=True))
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'a1_constants_a1_configuration.json')))
    assert abs(vals['urdf_mass'][0] - gold['mass']) < 1e-12 and abs(gold['mass'] - 13.741) < 1e-9
    assert np.abs(np.array(vals['urdf_Ir']) - np.array(gold['Ir']).reshape(-1)).max() < 1e-12
    hips = np.array([gold['hip_xy'][k] for k in ('FL', 'FR', 'RL', 'RR')]).reshape(-1)
    assert np.abs(np.array(vals['urdf_hip']) - hips).max() < 1e-12


@pytest.mark.gpu
def test_mpc_facade_runs_the_controller_protocol_like_the_ctypes_path(tmp_path):
    """The controller loop of tests/cpp/controller_driver.cpp (11 ticks, gait step every 5th: two GaitOpt + two LineSearch) through mpc::MPCSingleRigidBody /
    mpc::GaitOptimizer equals the same call sequence through the Python binding: same library underneath, so bit-identical."""
    cfg, exe = build_callsites(str(tmp_path))
    TICKS, F = 11, 5
    vals = parse_dump(subprocess.check_output([exe, '-', str(TICKS), str(F), str(tmp_path)], text=True))
    # header block of the log the program wrote through MPC::PrintStatLineToFile
    log = open(os.path.join(str(tmp_path), 'mpc_facade_log.txt')).read().splitlines()
    assert log[0] == '-' * 150 and 'MPC Statistics' in log[1] and log[2].startswith('MPC started at: ') and log[3] == 'Number of nodes: 20'
    assert len([l for l in log if l[:1].isdigit()]) == TICKS and all(len(l.rstrip()) <= 150 for l in log)
    s0 = np.array(cfg['srb_init'], float)
    ee0 = EE_NOMINAL
    g = host.BatchMPC.cold_start(cfg, s0, None, mode=(0.0, 0.0), initial_run=False)    # as mpc::MPCSingleRigidBody of the facade does (gap criterion for every solve)
    g.add_force_cost(cfg['force_cost'])
    g.create_initial_run(s0, ee0)
    gait = host.BatchGaitOptimizer(g)
    state, ee = s0, ee0.reshape(1, 12)
    traj = g.get_trajectory()[0]
    contact = traj.get_contacts(0.0)
    ready, n_ls, ls_cost = False, 0, 0.0
    for run in range(TICKS):
        t = run * cfg['integrator_dt']
        if run > 0:
            state = traj.get_states()[1]
            ee = np.array([traj.get_end_effector_location(e, t) for e in range(4)]).reshape(1, 12)
            contact = traj.get_contacts(t)
        g.adjust_for_current_contacts(t, np.array(contact, np.int32))
        if run % F == 0 and run > 0 and ready:
            imin, costs = gait.line_search(state, t, ee)
            ready = False; n_ls += 1; ls_cost = costs[0, imin[0]]
        elif (run + 1) % F == 0 and run > 0:
            g.get_real_time_update(state, t, ee)
            ready = g.status()[0][0] == 0
            if ready:
                gait.compute_sensitivity(); gait.compute_gradient(); gait.gradient(); gait.optimize_contact_times(t)
        else:
            g.get_real_time_update(state, t, ee); ready = False
        traj = g.get_trajectory()[0]
    avg = g.avg_cost()[0]
    tn = TICKS * cfg['integrator_dt']
    state = traj.get_states()[1]
    ee = np.array([traj.get_end_effector_location(e, tn) for e in range(4)]).reshape(1, 12)
    g.get_real_time_update(state, tn, ee)
    assert vals['copy_equal'] == [1.0] and vals['line_searches'] == [float(n_ls)] and n_ls == 2 and vals['run_num'] == [float(TICKS)]
    assert vals['no_match'] == [0.0]
    sz = g.sizes()[0]
    assert vals['n'] == [float(sz[0])] and vals['m'] == [float(sz[1])] and vals['quality'] == [float(g.status()[0][0])]
    assert np.array_equal(np.array(vals['x']), g.qp_solution()[0, :40])
    assert vals['cost'][0] == g.cost()[0] and vals['avg_cost'][0] == avg and vals['ls_cost'][0] == ls_cost
    assert vals['mass'][0] == cfg['mass'] and vals['manifold'] == [13.0]
    t2 = g.get_trajectory()[0]
    f = np.array([t2.get_force(e, tn + 0.013) for e in range(4)]).reshape(-1)
    p = np.array([t2.get_end_effector_location(e, tn + 0.013) for e in range(4)]).reshape(-1)
    assert np.array_equal(np.array(vals['force']), f) and np.array_equal(np.array(vals['pos']), p)
    assert np.array_equal(np.array(vals['contact_time']), np.concatenate(t2.get_contact_times()))
    assert np.array_equal(np.array(vals['box_center']), g.ee_box_center().reshape(-1))
    assert vals['viz'] == [5.0, 21.0]
    # MPC::PrintStats: one row per Solve since construction (10 of CreateInitialRun, the plain ticks, the final update), then the average time
    n_rows = 10 + (TICKS - n_ls) + 1
    assert vals['recorded'] == [float(n_rows)]
    stats = open(os.path.join(str(tmp_path), 'mpc_facade_stats.txt')).read().splitlines()
    assert stats[0] == '-' * 150 and 'MPC Statistics' in stats[1] and stats[2] == '-' * 150 and stats[3].split()[:2] == ['Solve', '#'] and stats[4] == '-' * 150
    rows = [l for l in stats if l[:1].isdigit()]
    assert [int(l.split()[0]) for l in rows] == list(range(n_rows)) and all(len(l.rstrip()) <= 150 for l in rows)
    assert all(('Solved' in l) or ('Max Iter' in l) for l in rows)
    assert stats[-1].startswith('Average compute time: ') and float(stats[-1].split(':')[1]) > 0
    last = rows[-1].split()
    assert abs(float(last[4]) - g.stats()[0, 0]) <= 1e-5 * max(1.0, abs(g.stats()[0, 0]))          # Alpha column of the last solve (%g precision)
    assert abs(float(last[5]) - g.cost()[0]) <= 1e-5 * abs(g.cost()[0])                             # Cost column
    # Trajectory::SplinesAsVec == the spline part of the decision vector the trajectory was written from; PrintTrajectoryToFile as coded
    n = int(sz[0]); nx = (cfg['num_nodes'] + 1) * 12
    assert len(vals['spline_vec']) == n - nx
    assert np.abs(np.array(vals['spline_vec']) - g.qp_solution()[0, nx:n]).max() <= 1e-12 * max(1.0, np.abs(g.qp_solution()[0, nx:n]).max())
    tr = open(os.path.join(str(tmp_path), 'mpc_facade_traj.txt')).read().splitlines()
    assert tr[0] == 'states: ' and tr[22] == 'force spline: ' and tr[23] == 'position spline: ' and tr[24] == 'timings: ' and tr[25] == 'spline vec: '
    st_file = np.array([[float(v) for v in l.split()] for l in tr[1:22]])
    assert st_file.shape == (21, 13) and np.allclose(st_file, t2.get_states(), rtol=2e-5, atol=1e-6)
    assert len({len(l) for l in tr[1:22]}) == 1                       # Eigen's aligned columns: every row has the same width
    assert np.allclose([float(l) for l in tr[26:26 + n - nx]], vals['spline_vec'], rtol=2e-5, atol=1e-6) and len(tr) == 26 + n - nx


def check_urdf_constants(vals, gold):
    assert abs(vals['urdf_mass'][0] - gold['mass']) < 1e-12
    assert np.abs(np.array(vals['urdf_Ir']) - np.array(gold['Ir']).reshape(-1)).max() < 1e-11
    hips = np.array([gold['hip_xy'][k] for k in ('FL', 'FR', 'RL', 'RR')]).reshape(-1)
    assert np.abs(np.array(vals['urdf_hip']) - hips).max() < 1e-12
    legs = np.array([gold['leg_origins'][k] for k in ('FL', 'FR', 'RL', 'RR')]).reshape(-1)
    assert np.array_equal(np.array(vals['urdf_leg']), legs)
    assert np.abs(np.array(vals['urdf_body_mass']) - np.array([b['mass'] for b in gold['body_model']])).max() < 1e-12
    assert np.abs(np.array(vals['urdf_body_com']) - np.array([b['com'] for b in gold['body_model']]).reshape(-1)).max() < 1e-12
    assert np.abs(np.array(vals['urdf_body_inertia']) - np.array([b['inertia'] for b in gold['body_model']]).reshape(-1)).max() < 1e-12


def test_row_f3_call_sites_compile_and_the_urdf_reader_gives_the_kinematics_and_body_constants(tmp_path):
    """The methods of controllers/mpc_controller.cpp:160-226 and :414-511 (targets from the trajectory, the whole-body QP), called in that order by
    the builder-written tests/cpp/wbc_driver.cpp, compile warning-free against include/mpc_facade/controllers.h (controller::QPControl,
    mpc::SingleRigidBodyModel with the reference's signatures); the facade's URDF reader gives the leg geometry and the thirteen merged bodies
    the library needs -- from a URDF written out of the committed constants and from the reference's models/a1_description/urdf/a1.urdf
    (tests/golden/a1.urdf), whose fixed links (imu, rotors ... feet) it has to merge itself."""
    cfg, exe = build_wbc_callsites(str(tmp_path))
    urdf = os.path.join(str(tmp_path), 'from_constants.urdf')
    gold = write_urdf_from_golden(urdf)
    check_urdf_constants(parse_dump(subprocess.check_output([exe, urdf, '0'], text=True)), gold)
    check_urdf_constants(parse_dump(subprocess.check_output([exe, A1_URDF, '0'], text=True)), gold)


@pytest.mark.gpu
def test_row_f3_facade_runs_the_control_tick_like_the_ctypes_path(tmp_path):
    """MPCController::ComputeControlAction through controller::QPControl / mpc::SingleRigidBodyModel / mpc::MPCSingleRigidBody (two single
    IK calls and the host-side interpolation of the reference's text) against the fused batch entries of the Python binding
    (srbm_get_targets_from_traj, srbm_qp_control) on the same protocol: targets <= 1e-9, control action <= 1e-6 relative."""
    cfg, exe = build_wbc_callsites(str(tmp_path))
    urdf = os.path.join(str(tmp_path), 'from_constants.urdf')
    gold = write_urdf_from_golden(urdf)
    TICKS = 5
    vals = parse_dump(subprocess.check_output([exe, urdf, str(TICKS)], text=True))
    assert vals['tick_status'] == [0.0] * TICKS and vals['run_num'] == [float(TICKS)]
    s0 = np.array(cfg['srb_init'], float)
    q0 = np.array(gold['source']['init_config'], float)
    g = host.BatchMPC.cold_start(cfg, s0, None, mode=(0.0, 0.0), initial_run=False)    # as mpc::MPCSingleRigidBody of the facade does (gap criterion for every solve)
    g.add_force_cost(cfg['force_cost'])
    ee0 = g.forward_kinematics(q0)[0]
    ee0[:, 2] = 0
    g.create_initial_run(s0, ee0.reshape(1, 12))
    traj = g.get_trajectory()[0]
    for i in range(3):
        t = i * cfg['integrator_dt']
        state = traj.get_states()[1]
        ee = np.array([traj.get_end_effector_location(e, t) for e in range(4)]).reshape(1, 12)
        g.get_real_time_update(state, t, ee)
        traj = g.get_trajectory()[0]
    t0 = traj.init_time
    assert vals['t0'][0] == t0
    q_des = q0.reshape(1, 19).copy(); v_des = np.zeros((1, 18))
    for k in range(TICKS):
        time = t0 + 1e-3 * (k + 1)
        q_meas = q_des.copy(); q_meas[0, 7:] += 0.01 * ((np.arange(12) % 3) - 1)
        v_meas = 0.9 * v_des
        q_des, v_des, f_des, st = g.get_targets_from_traj(time, q_des)
        assert st[0] == 0
        _, _, con = g.eval_trajectory(time)
        fd = np.zeros((1, 12)); sel = f_des[0][con[0] > 0].reshape(-1); fd[0, :sel.size] = sel
        ctl, sol, stq, itq = g.qp_control(q_meas, v_meas, con, q_des, v_des, fd)
        assert stq[0] <= 1
    assert np.array_equal(np.array(vals['contact']), con[0].astype(float))
    assert np.abs(np.array(vals['q_des']) - q_des[0]).max() < 1e-9, np.abs(np.array(vals['q_des']) - q_des[0]).max()
    assert np.abs(np.array(vals['v_des']) - v_des[0]).max() < 1e-6 * max(1.0, np.abs(v_des).max())
    assert np.abs(np.array(vals['control']) - ctl[0]).max() < 1e-6 * max(1.0, np.abs(ctl).max()), np.abs(np.array(vals['control']) - ctl[0]).max()


# ---------------- the callers outside the controller: gait_opt_playground.cpp, mpc_test.cpp "Model Partials", the model's maps ----------------
def build_playground(tmpdir):
    cfg = host.load_config('a1_configuration')
    host.build()
    write_cfg_inc(cfg, os.path.join(tmpdir, 'cfg.inc'))
    exe = os.path.join(tmpdir, 'playground_driver')
    libdir = os.path.dirname(host.LIB_PATH)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-I', EIGEN_INC, '-I', tmpdir,
                           os.path.join(CPP, 'playground_driver.cpp'), '-o', exe, '-L', libdir, '-lsrbm_rti', '-Wl,-rpath,' + libdir])
    return cfg, exe


def test_playground_driver_compiles_against_the_mpc_facade(tmp_path):
    """The builder-written behaviour driver of test/gait_opt_playground.cpp (RunGaitOpt, PrintContactSched, MPCWithFixedPosition: GetFullTargetState,
    GetQPData with its size asserts, GetModifiedCost, PrintStats, CreateVizData, GetEEBoxCenter) and of SECTION("Model Partials") of
    test/mpc_test.cpp:114-270 (QPPartials read as matrices, finite differences of GetQPData().sparse_constraint_) -- tests/cpp/playground_driver.cpp --
    compiles warning-free against include/mpc_facade/mpc.h and links against the C-ABI library."""
    cfg, exe = build_playground(str(tmp_path))
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_playground_protocol_and_the_reference_partials_test_through_the_facade(tmp_path):
    """Runs tests/cpp/playground_driver.cpp: (1) the reference's own "Model Partials" test passes on the device through mpc::QPPartials / mpc::QPData
    (every dynamics / force-box / friction-cone entry within 1e-4 of the finite difference, all contact times with idx >= 1);
    (2) the QP sizes are stable across every solve of the playground loop (the asserts of gait_opt_playground.cpp:129-130);
    (3) GetFullTargetState, the costs and the optimised schedule equal the same call sequence through the Python binding."""
    cfg, exe = build_playground(str(tmp_path))
    urdf = os.path.join(str(tmp_path), 'from_constants.urdf')
    gold = write_urdf_from_golden(urdf)
    ITER = 6
    vals = parse_dump(subprocess.check_output([exe, urdf, str(ITER)], text=True))
    # model maps (mpc_controller.cpp:60, :258)
    tgt = np.array(cfg['srb_target'], float)
    assert np.abs(np.array(vals['des_alg']) - host.manifold_to_tangent(tgt)).max() < 1e-15
    assert np.abs(np.array(vals['des_back']) - tgt).max() < 1e-14
    assert np.abs(np.array(vals['Ir_w']) - np.array(gold['Ir']).reshape(3, 3) @ np.array([0.3, -0.2, 0.1])).max() < 1e-12
    # (1) test/mpc_test.cpp:114-270
    assert vals['partials_checked'][0] >= 12 and vals['partials_worst_fd'][0] < 1e-4, vals['partials_worst_fd']
    # (2)
    assert vals['qp_same_size'] == [1.0] * ITER and len(set(vals['qp_n'])) == 1 and vals['qp_n'][0] == 372.0
    # (3) the same protocol through ctypes
    s0 = np.array(cfg['srb_init'], float)
    ee0 = EE_NOMINAL
    g = host.BatchMPC.cold_start(cfg, s0, None, mode=(0.0, 0.0), initial_run=False)
    g.add_force_cost(cfg['force_cost'])
    g.create_initial_run(s0, ee0)
    gait = host.BatchGaitOptimizer(g)
    traj = g.get_trajectory()[0]
    state = np.array(gold['source']['init_config'], float)
    sched_before = np.concatenate(traj.get_contact_times())
    ik, costs, gait_steps = [], [], 0
    for i in range(ITER):
        t = 0.0                                   # fixed_pos = true (gait_opt_playground.cpp:85-87,364-365)
        cur = g.get_trajectory()[0]
        ee_now = np.array([cur.get_end_effector_location(e, t) for e in range(4)])
        q, _, st = g.inverse_kinematics(cur.get_states()[cur.get_node(t)], ee_now.reshape(1, 12), state)
        assert st[0] == 0
        state = q[0]; ik.append(state)
        ee = np.array([traj.get_end_effector_location(e, t) for e in range(4)]).reshape(1, 12)
        if i % 2 == 0 and g.status()[0][0] == 0:
            gait.compute_sensitivity(); gait.compute_gradient()
            _, valid = gait.gradient()
            assert valid[0] == 1
            gait.optimize_contact_times(t)
            xk, counts = gait.contact_times(); step = gait.step()
            new = xk[0] + step[0]
            times = np.zeros((1, 4, 8)); off = 0
            ct = g.get_trajectory()[0].get_contact_times()
            for e in range(4):
                for k in range(counts[0, e]):
                    v = new[off + k]
                    if k > 0:
                        d = times[0, e, k - 1] - v
                        if 0 < d <= 1e-3: v = times[0, e, k - 1]
                    times[0, e, k] = v
                off += counts[0, e]
            g.update_contact_times(times)
            gait_steps += 1
        g.get_real_time_update(traj.get_states()[0], t, ee)
        traj = g.get_trajectory()[0]
        costs.append(g.cost()[0])
    assert vals['gait_steps'][0] == gait_steps and gait_steps == 3
    assert np.array_equal(np.array(vals['modified_cost']), np.array(costs))
    assert np.array_equal(np.array(vals['ik_state']), np.concatenate(ik))
    assert np.array_equal(np.array(vals['sched_before']), sched_before)
    sched_after = np.concatenate(traj.get_contact_times())
    assert np.array_equal(np.array(vals['sched_after']), sched_after) and not np.array_equal(sched_after, sched_before)
    assert len(vals['target_config']) == 7 and np.array_equal(np.array(vals['target_config']), traj.get_states()[1][6:])
    assert len(vals['force_target']) in (6, 12)
