"""The typed ctypes bindings held together (no GPU): host.PROTOTYPES and oracle_py.PROTOTYPES against the symbols of the built libraries and against
the C text (include/srbm_rti.h, csrc/srbm_capi.hip, oracle/oracle_capi.cpp); the struct mirrors and the restated constants against what g++ makes
of the header; wrong calls refused before they reach C; every public method of the binding converting its arguments under the declared types."""
import ctypes as C
import functools
import inspect
import io
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py
from srbm_loader import host, ROOT

HEADER = os.path.join(ROOT, 'include', 'srbm_rti.h')
CAPI = os.path.join(ROOT, 'bilevel-gait-gen_amd', 'csrc', 'srbm_capi.hip')
ORACLE_CAPI = os.path.join(ROOT, 'oracle', 'oracle_capi.cpp')
ORACLE_TYPES = dict(host.C_TYPES, **{'orc_config*': C.POINTER(oracle_py.OrcConfig)})
DP, IP, VP = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p


@pytest.fixture(scope='module')
def libs():
    host.build()
    return host.lib(), host.lib(True)


# ---- a. table == library ----
def exported(path, prefix):
    out = subprocess.check_output(['nm', '-D', '--defined-only', path], text=True)
    return {f[2] for f in (l.split() for l in out.splitlines()) if len(f) == 3 and f[1] == 'T' and f[2].startswith(prefix)}


def test_table_equals_the_exported_symbols(libs):
    for path in (host.LIB_PATH, host.LIB_PATH_LARGE):
        syms = exported(path, 'srbm_')
        assert len(syms) >= 118 and syms == set(host.PROTOTYPES), (os.path.basename(path), sorted(syms ^ set(host.PROTOTYPES)))
    syms = exported(os.path.join(oracle_py.ORACLE_DIR, 'liboracle.so'), 'orc_')
    assert len(syms) >= 56 and syms == set(oracle_py.PROTOTYPES), sorted(syms ^ set(oracle_py.PROTOTYPES))


def test_declare_raises_on_a_symbol_the_library_lacks(libs):
    with pytest.raises(AttributeError, match='srbm_no_such_entry'):
        host.declare(C.CDLL(host.LIB_PATH), {'srbm_no_such_entry': (C.c_int, ())})


# ---- b. table == C text ----
def c_key(decl, named):
    """the key of host.C_TYPES for one C declarator: const dropped, a parameter whose name ends in _dev is a device pointer"""
    decl = ' '.join(re.sub(r'\bconst\b', ' ', decl).split())
    name = ''
    if named:
        decl, name = re.fullmatch(r'(.*?)\s*(\w+)', decl).groups()
    decl = decl.replace(' *', '*')
    if name.endswith('_dev'):
        assert decl.endswith('*') and not decl.endswith('**'), (decl, name)
        return 'dev*'
    return decl


def parse_c(path, prefix, definitions, start=None):
    """name -> (return key, [argument keys]) of every `ret prefix_name(args);` (or `{` for definitions) that begins a line"""
    text = open(path).read()
    if start is not None:
        text = text[text.index(start):]
    text = re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    ret = r'(?:const\s+)?(?:char|void|int|long|double|srbm_batch)\s*\**'
    found = {}
    for m in re.finditer(r'^(%s)\s*\b(%s\w+)\s*\(([^)]*)\)\s*%s' % (ret, prefix, r'\{' if definitions else ';'), text, flags=re.M):
        args = [a for a in m.group(3).split(',') if a.strip() not in ('', 'void')]
        assert m.group(2) not in found, m.group(2)
        found[m.group(2)] = (c_key(m.group(1), False), [c_key(a, True) for a in args])
    return found


def check_against(table, parsed, types):
    for name, (ret, args) in parsed.items():
        restype, argtypes = table[name]
        assert restype is types[ret], (name, ret)
        assert len(argtypes) == len(args), (name, args)
        for i, a in enumerate(args):
            assert argtypes[i] is types[a], (name, i, a)


def test_the_mapping_from_c_to_ctypes():
    """the one dict of the binding, restated: scalars, typed host pointers, c_void_p for handles / void* / device pointers, pointers to the mirrors;
    srbm_leg_kinematics* is THE EXCEPTION -- it has no mirror and is declared as the flat double array host.py passes"""
    assert host.C_TYPES == {
        'void': None, 'int': C.c_int, 'double': C.c_double, 'long': C.c_long, 'char*': C.c_char_p, 'char**': C.POINTER(C.c_char_p),
        'double*': DP, 'int*': IP, 'long long*': C.POINTER(C.c_longlong),
        'srbm_batch*': VP, 'srbm_gait*': VP, 'ncclComm_t': VP, 'void*': VP, 'dev*': VP,
        'srbm_batch**': C.POINTER(VP), 'srbm_gait**': C.POINTER(VP), 'ncclComm_t*': C.POINTER(VP),
        'srbm_mpc_info*': C.POINTER(host.MPCInfo), 'srbm_model*': C.POINTER(host.Model), 'srbm_wbc_model*': C.POINTER(host.WbcModel),
        'srbm_trajectory*': C.POINTER(host.Trajectory),
        'srbm_leg_kinematics*': DP}


def test_table_equals_the_header_and_the_definitions():
    hdr = parse_c(HEADER, 'srbm_', False)
    assert len(hdr) >= 105                                # a broken pattern must not pass on nothing
    declared = set(re.findall(r'\b(srbm_[a-z_0-9]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)))
    assert set(hdr) == declared and declared <= set(host.PROTOTYPES)      # every function the header declares is parsed and is in the table
    check_against(host.PROTOTYPES, hdr, host.C_TYPES)
    defs = parse_c(CAPI, 'srbm_', True, start='extern "C" {')
    assert len(defs) >= 118 and set(defs) == set(host.PROTOTYPES), sorted(set(defs) ^ set(host.PROTOTYPES))
    check_against(host.PROTOTYPES, defs, host.C_TYPES)
    # the device pointers are exactly the pointer parameters of the *_dev entries and of the RCCL all-gather
    dev = {n for n, (_, a) in hdr.items() if 'dev*' in a}
    assert dev == {n for n in hdr if n.endswith('_dev')} | {'srbm_allgather_results'}


def test_oracle_table_equals_its_definitions():
    defs = parse_c(ORACLE_CAPI, 'orc_', True, start='extern "C" {')
    assert len(defs) >= 56 and set(defs) == set(oracle_py.PROTOTYPES), sorted(set(defs) ^ set(oracle_py.PROTOTYPES))
    check_against(oracle_py.PROTOTYPES, defs, ORACLE_TYPES)
    assert oracle_py.PROTOTYPES['orc_mpc_create'] == (VP, (C.POINTER(oracle_py.OrcConfig),))
    assert {n for n, (r, _) in oracle_py.PROTOTYPES.items() if r is C.c_double} == {
        'orc_spline_value_at', 'orc_spline_end_time', 'orc_spline_start_time', 'orc_spline_partial_wrt_time', 'orc_mpc_ee_value', 'orc_mpc_init_time'}


# ---- c, d. struct mirrors and constants == what g++ makes of the header ----
MIRRORS = {'srbm_mpc_info': host.MPCInfo, 'srbm_model': host.Model, 'srbm_wbc_model': host.WbcModel, 'srbm_trajectory': host.Trajectory}
CONSTANTS = {'SRBM_TRAJ_KMAX': host.KMAX, 'SRBM_TRAJ_NODES_MAX': host.NODES_MAX, 'SRBM_STEP_LOG_DOUBLES': host.STEP_LOG_DOUBLES,
             'SRBM_GAIT_NV': host.BatchGaitOptimizer.NV, 'SRBM_GAIT_LS_SIZE': host.BatchGaitOptimizer.LS_SIZE,
             'SRBM_FAST_TOL_STEP': host.FAST_TOL_STEP, 'SRBM_FAST_START_MU': host.FAST_START_MU,
             'SRBM_RCCL_UNIQUE_ID_BYTES': host.RCCL_UNIQUE_ID_BYTES}


@pytest.fixture(scope='module')
def header_facts(tmp_path_factory):
    """lines `key value...` printed by a program that includes the header: sizeof and per member offsetof / sizeof of the mirrored structs, the #defines"""
    d = tmp_path_factory.mktemp('abi')
    body = ['#include <cstddef>', '#include <cstdio>', '#include "srbm_rti.h"', 'int main() {']
    for s, cls in MIRRORS.items():
        body.append('    std::printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in cls._fields_:
            body.append('    std::printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    body.append('    std::printf("srbm_leg_kinematics %zu\\n", sizeof(srbm_leg_kinematics));')
    for k in CONSTANTS:
        body.append('    std::printf("%s %%.17g\\n", (double)%s);' % (k, k))
    body += ['    return 0;', '}']
    src, exe = os.path.join(d, 'abi_facts.cpp'), os.path.join(d, 'abi_facts')
    open(src, 'w').write('\n'.join(body) + '\n')
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-o', exe, src])
    return {l.split()[0]: l.split()[1:] for l in subprocess.check_output([exe], text=True).splitlines()}


def test_struct_mirrors_have_the_layout_of_the_header(header_facts):
    for s, cls in MIRRORS.items():
        assert int(header_facts[s][0]) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert [int(v) for v in header_facts['%s.%s' % (s, f)]] == [d.offset, d.size], (s, f)
    # the member names of each struct in the header, in order, are the mirror's (a member the mirror lacks would otherwise show only in sizeof)
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    for s, cls in MIRRORS.items():
        members = re.search(r'typedef struct %s \{(.*?)\} %s;' % (s, s), text, flags=re.S).group(1)
        names = [re.match(r'\w+', d.strip()).group(0) for stmt in members.split(';') if stmt.strip()
                 for d in re.sub(r'^\s*(int|double)\b', '', stmt.strip()).split(',')]
        assert names == [f for f, _ in cls._fields_], s
    # the struct without a mirror is the flat array it is passed as
    assert int(header_facts['srbm_leg_kinematics'][0]) == 4 * 4 * 3 * C.sizeof(C.c_double)


def test_restated_constants_equal_the_header(header_facts):
    for k, v in CONSTANTS.items():
        assert float(header_facts[k][0]) == v, k


# ---- e. wrong calls are refused before they reach C ----
def swing_first_trajectory(scale):
    """the record of test_trajectory_record_layout_and_host_evaluation (test_abi_and_host.py) with its knot times multiplied by `scale`"""
    t = host.Trajectory()
    t.num_states = 21; t.node_dt = 0.05 * scale; t.swing_height = 6.0; t.foot_offset = 0.0
    times = [0.0, 0.1, 0.2, 0.2 + 0.2 / 3, 0.2 + 0.4 / 3, 0.4, 0.5, 0.6, 0.6 + 0.2 / 3, 0.6 + 0.4 / 3, 0.8]
    kinds = [0, 3, 1, 2, 2, 0, 3, 1, 2, 2, 0]
    for ee in range(4):
        t.nk[ee] = len(times)
        for k, (tt, kd) in enumerate(zip(times, kinds)):
            t.knot_time[ee][k] = tt * scale; t.knot_kind[ee][k] = kd
    for k, v in zip([0, 2, 5, 7, 10], [0.0, 2.0, 2.0, 7.0, 7.0]):
        t.pos_xy[0][0][k] = v
    return t


def test_wrong_calls_are_refused_and_numbers_are_converted(libs):
    L = libs[0]
    a64, a32 = np.zeros(4), np.zeros(4, np.int32)
    with pytest.raises(C.ArgumentError):
        L.srbm_rti_advance(None, 'zero', 1)                       # a str for an int
    with pytest.raises(C.ArgumentError):
        L.srbm_rti_advance(None, 0, 1.0)                          # a float for an int
    with pytest.raises(C.ArgumentError):
        L.srbm_get_cost(None, a32.ctypes.data_as(IP))             # an int32 array for a double*
    with pytest.raises(C.ArgumentError):
        L.srbm_get_cost(None, a64.ctypes.data)                    # a bare integer for a host double*
    with pytest.raises(C.ArgumentError):
        L.srbm_get_sizes(None, a64.ctypes.data_as(DP))            # and a double array for an int*
    # a Python int for a double arrives as that double: the stance of the foot begins at t = 1 (knot 2, x = 2); untyped, the callee would read
    # whatever the floating-point argument register held
    t = swing_first_trajectory(5.0)
    res = []
    for time in (1, 1.0, np.float32(1.0), np.int64(1)):
        f = (C.c_double * 3)(); p = (C.c_double * 3)(); c = C.c_int(-1)
        assert L.srbm_trajectory_eval(C.byref(t), 0, time, f, p, C.byref(c)) == 0
        res.append((list(f), list(p), c.value))
    assert res[0][1][0] == 2.0 and res[0][2] == 1 and all(r == res[0] for r in res)
    # an int for the double of a setter is accepted by the types and reaches the callee, which refuses the null handle (what arrives is shown above)
    assert L.srbm_add_force_cost(None, 1) < 0 and 'bad arguments' in L.srbm_last_error().decode()
    # return types: a pointer comes back whole (None for NULL), a long as an int, a string as bytes
    assert L.srbm_stream(None) is None and L.srbm_gait_debug_candidates(None) is None
    assert L.srbm_bytes_per_instance() > 2 ** 16 and isinstance(L.srbm_last_error(), bytes)


# ---- f. every public method converts ----
HANDLE = 0x7f1234567890               # a handle / device address above 2^32


class StandIn:
    """In place of a loaded library: every entry of the table checks the argument count, converts each argument as ctypes would on the call
    (argtypes[i].from_param) and reports success without touching its outputs."""

    def __init__(self, table, capacity):
        self.capacity, self.calls = capacity, []
        for name, (restype, argtypes) in table.items():
            setattr(self, name, functools.partial(self._call, name, restype, argtypes))

    def _call(self, name, restype, argtypes, *args):
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for i, (t, a) in enumerate(zip(argtypes, args)):
            try:
                t.from_param(a)
            except (TypeError, C.ArgumentError) as e:
                raise AssertionError('%s: argument %d: %s' % (name, i, e))
        self.calls.append(name)
        return {C.c_void_p: HANDLE, C.c_char_p: b'stand-in'}.get(restype, 0)


def public_methods(cls):
    return {n for n, f in inspect.getmembers(cls, callable) if not n.startswith('_')}


def test_every_public_method_converts_under_the_declared_types(monkeypatch):
    fake = StandIn(host.PROTOTYPES, dict(N=50, nu=160, samples=120, knots=32))
    fake_large = StandIn(host.PROTOTYPES, dict(N=100, nu=240, samples=200, knots=32))
    monkeypatch.setitem(host._libs, host.LIB_PATH, fake)
    monkeypatch.setitem(host._libs, host.LIB_PATH_LARGE, fake_large)
    cfg = host.load_config('a1_configuration')
    B = 3
    s0 = np.array(cfg['srb_init'], float); S = np.tile(s0, (B, 1))
    ee = np.array([[0.2, 0.2, 0], [0.2, -0.2, 0], [-0.2, 0.2, 0], [-0.2, -0.2, 0]], float); EE = np.tile(ee, (B, 1, 1))
    q19 = np.zeros(19); q19[6] = 1.0
    dev = [HANDLE + 4096 * i for i in range(10)]

    g = host.BatchMPC(cfg, B)
    assert g.L is fake and {'srbm_batch_create', 'srbm_set_leg_kinematics', 'srbm_set_wbc_model'} <= set(fake.calls)
    assert host.BatchMPC(dict(cfg, num_nodes=80), 1).L is fake_large
    g.h = C.c_void_p(HANDLE)               # (the stand-in does not write its outputs)
    trajs = g.get_trajectory()
    cases = {          # method -> argument tuples, in the shapes the GPU tests use: scalar and per-instance inputs, integer device addresses, None
        'instance_model': [(1,)], 'clone': [()], 'get_trajectory': [(), (1, 2)],
        'set_warm_start_trajectory': [(trajs,), ([host.Trajectory(), host.Trajectory()], 1)],
        'eval_trajectory': [(0.05,), (np.full(B, 0.05),)], 'ee_box_center': [()], 'cost': [()], 'merit': [()], 'avg_cost': [()],
        'add_force_cost': [(1,), (0.001,), (np.float64(2.0),)], 'status_accumulated': [()], 'clear_status_accumulators': [()], 'executed_mfma': [()],
        'result_record_doubles': [()], 'add_quadratic_tracking_cost': [(np.zeros(12), np.eye(12))], 'set_quadratic_final_cost': [(np.eye(12),)],
        'set_linear_final_cost': [(np.zeros(12),)], 'add_quadratic_tracking_cost_each': [(1, np.zeros((2, 12)), np.zeros((2, 12, 12)))],
        'set_quadratic_final_cost_each': [(0, np.zeros((B, 12, 12)))], 'set_linear_final_cost_each': [(0, np.zeros((B, 12)))],
        'add_force_cost_each': [(0, [0.1, 0.2, 0.3])], 'set_solver_step_rule': [(0, 0), (1e-5, 0.1), (0.0,)], 'enable_fast_termination': [()],
        'enable_lower_start': [()], 'solve_flags': [()], 'solver_step_rule': [()], 'solver_counters': [()],
        'set_state_trajectory_warm_start': [(s0,), (S,)], 'set_solver_tolerances': [host.REFERENCE_SOLVER_SETTINGS, (1e-8, 1e-8, 1e-8, 50.0)],
        'create_initial_run': [(s0, ee), (S, EE)], 'get_real_time_update': [(s0, 0.0, ee), (S, np.zeros(B), EE), (s0, 0, ee)],
        'get_real_time_update_dev': [tuple(dev[:3])], 'rti_advance': [(0, 1), (np.int64(3), 20.0)], 'rti_advance_unfused': [(0, 2)],
        'plant_set_state': [(s0,), (S,)], 'plant_state': [()], 'plant_set_push': [(), (0.1, np.ones(6)), (np.full(B, 0.1), np.ones((B, 6)))],
        'closed_loop_advance': [(0, 5), (0, 5, 4, True)], 'step_log_enable': [(8,)], 'step_log_reset': [()], 'step_log_count': [()],
        'step_log': [(), (1, 2)], 'step_log_copy_dev': [(dev[0],), (dev[0], 1, 3)], 'synchronize': [()], 'stream': [()],
        'update_contact_times': [(np.zeros((B, 4, 5)),)], 'adjust_for_current_contacts': [(0.0, [1, 1, 0, 1]), (np.zeros(B), np.ones((B, 4), int))],
        'forward_kinematics': [(q19,)], 'inverse_kinematics': [(s0, ee, q19), (S, EE, np.tile(q19, (B, 1)))],
        'get_targets_from_traj_dev': [tuple(dev[:5])], 'eval_trajectory_dev': [tuple(dev[:4])], 'qp_control_dev': [tuple(dev[:9])],
        'get_targets_from_traj': [(0.0, q19), (np.zeros(B), np.tile(q19, (B, 1)))],
        'qp_control': [(q19, np.zeros(18), [1, 1, 1, 1], q19, np.zeros(18), np.zeros(12)), (q19, np.zeros(18), np.ones((B, 4), int), q19, np.zeros(18), np.zeros(12), True)],
        'print_stat_header': [(io.StringIO(),)], 'print_stat_line': [(io.StringIO(), 1, 0.5)], 'enable_kernel_timing': [(16,)], 'kernel_timing': [()],
        'kernel_timings': [(), (8,)], 'debug_launch_info': [()], 'work_counters': [()], 'pack_results_dev': [(dev[0], 1000)],
        'rccl_unique_id': [()], 'rccl_comm_init_rank': [(1, 0, bytes(host.RCCL_UNIQUE_ID_BYTES))], 'rccl_comm_destroy': [(HANDLE,)],
        'allgather_results': [(HANDLE, dev[0])], 'pack_results': [()], 'sizes': [()], 'status': [()], 'stats': [()], 'qp_cost': [()],
        'qp_solution': [()], 'raw_qp_minimiser': [()], 'dual_solution': [()], 'trajectory_states': [()], 'knots': [(0,)], 'export_qp': [(0,)],
        'param_partials': [(0, 1, 2)]}
    called_below = {'from_configs', 'cold_start', 'close'}
    assert set(cases) | called_below == public_methods(host.BatchMPC)
    for name, argsets in cases.items():
        for args in argsets:
            getattr(g, name)(*args)
    assert g.stream() == HANDLE and g.rccl_comm_init_rank(1, 0, bytes(128)) is None and g.qp_solution().shape == (B, 21 * 12 + 160)
    assert g.dual_solution()[0].shape == (B, 21 * 12 + 6 * 120 + 16 * 17 + 16) and g.clone().h.value is None

    h = host.BatchMPC.from_configs([dict(cfg, mass=cfg['mass'] + i, force_cost=1e-3 * (i + 1)) for i in range(B)])
    assert h.batch == B and 'srbm_batch_create_each' in fake.calls
    for c in (host.BatchMPC.cold_start(cfg, S, EE), host.BatchMPC.cold_start([cfg, cfg], S[:2], EE[:2], mode=(host.FAST_TOL_STEP, host.FAST_START_MU)),
              host.BatchMPC.cold_start(dict(cfg, num_nodes=80), s0, ee, mode=(0, 0.1), initial_run=False)):
        assert c.batch in (1, 2, B)

    go = host.BatchGaitOptimizer(g)
    go.g = C.c_void_p(HANDLE)
    gait_cases = {'set_contact_times_from_trajectory': [()], 'contact_times': [()], 'compute_sensitivity': [()], 'sensitivity': [()],
                  'compute_gradient': [()], 'gradient': [()], 'set_gradient': [(np.zeros(8),), (np.zeros((B, 32)), np.ones(B, np.int32))], 'optimize_contact_times': [(0.25,), (np.full(B, 0.25),)], 'lp_result': [()],
                  'rti_advance': [(0, 10, 5)], 'set_step': [(np.zeros(8),), (np.zeros((B, 32)),)], 'step': [()],
                  'line_search': [(s0, 0.25, ee), (S, np.full(B, 0.25), EE)], 'candidates': [()], 'candidate_status': [()]}
    assert set(gait_cases) | {'close'} == public_methods(host.BatchGaitOptimizer)
    for name, argsets in gait_cases.items():
        for args in argsets:
            getattr(go, name)(*args)
    v = go.candidates()
    assert v.h.value == HANDLE and v.batch == B * go.LS_SIZE and v.status()[0].shape == (B * go.LS_SIZE,)
    assert go.sensitivity().shape == (B, 2 * 21 * 12 + 160 + 6 * 120 + 16 * 17 + 16) and go.candidate_status()[0].shape == (B, go.LS_SIZE)

    # the module functions and the host evaluation of a record go through the same table
    t = host.Trajectory()
    t.get_force(0, 0), t.get_end_effector_location(1, 0.5), t.get_contacts(np.float64(0.5))
    host.manifold_to_tangent(s0), host.dense_row_placement(20, 100, 30), host.dense_row_placement(80, 200, 60, large=True)

    go.close(); g.close(); h.close()
    assert not g.h and {'srbm_gait_destroy', 'srbm_batch_destroy'} <= set(fake.calls)
    # every entry that host.py names was converted at least once (but the two that only a real library sees: lib() asks it for its capacity, and
    # the error text is read after a failure)
    named = set(re.findall(r'\.(srbm_\w+)\(', open(os.path.join(ROOT, 'bilevel-gait-gen_amd', 'host.py')).read()))
    assert len(named) >= 78 and named - {'srbm_get_capacity', 'srbm_last_error'} <= set(fake.calls), sorted(named - set(fake.calls))


def test_nothing_but_declare_sets_a_return_or_argument_type():
    for d in ('bilevel-gait-gen_amd', 'tests', 'scripts'):
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            if f.endswith('.py') and f != os.path.basename(__file__):
                hits = [l for l in open(os.path.join(ROOT, d, f)).read().splitlines() if re.search(r'\.(restype|argtypes)\b', l)]
                assert len(hits) == (1 if f == 'host.py' else 0), (f, hits)
