"""The device-resident step log (include/srbm_rti.h: srbm_step_log_*; csrc/srbm_steplog.hiph): one record per (step, instance) of a launch.

A K-step launch leaves only its last solve in the read-back entries.  With a log enabled every solve also writes a record: the logged twins of the
multi-step kernels write it after the update phase of each step, the one-step entries through srbm_k_step_log.  What is held here, all of it
BITWISE (tobytes), in the clone pattern of tests/test_gpu_launch_equivalence.py:

    * the records of a chain of one-step launches, of one K-step launch and of a split launch are the same bytes;
    * every field of a record equals what the read-back entries give after the one-step launch of that solve: status, error bits, solve flags,
      sizes, stats, QP cost, merit dd, the merit derived on the host, the inputs handed to the solve (plant state, or node 1 of the previous
      trajectory, and the previous trajectory's foot locations), and srbm_eval_trajectory of the new trajectory at its init_time;
    * a logging batch and a non-logging one end with the same snapshot: logging changes no result;
    * the step queues (a batch larger than the chip) and the LARGE build's srbm_rti_fused_long write the same records as the chain;
    * the cursor, the refusals (capacity, slot ranges, no log), clones, the device-to-device copy and the statistics rows made from records."""
import ctypes as C
import io

import numpy as np
import pytest

from closed_loop_kit import chip_cu_count
from gpu_kit import advance, assert_bitwise, same_bytes, snapshot
from oracle_py import load_config
from srbm_loader import host
from srbm_loader.workloads import config_b_instance, instances

pytestmark = pytest.mark.gpu
MODE = (0.0, 0.1)           # lower-start attempts: solve flags other than 0 in the open-loop protocol
SUBSTEPS = 4
F = host.STEP_LOG_FIELDS


def step(g, closed, first, steps):
    if closed:
        g.closed_loop_advance(first, steps, SUBSTEPS, True)
    else:
        advance(g, False, first, steps)


def cold_start(cfg, B, large=None):
    """a batch after its cold start, with a plant and pushes at 2.5 dt on instances 0 and 1 (the open-loop protocol does not look at them)"""
    states, ees = instances(cfg, config_b_instance, B)
    g = host.BatchMPC.cold_start(cfg, states, ees, mode=MODE, large=large)
    g.plant_set_state(states)
    imp = np.zeros((B, 6)); imp[0, 0] = 0.4; imp[1, 1] = -0.3
    push_time = np.full(B, 1e9); push_time[:2] = 2.5 * cfg['integrator_dt']
    g.plant_set_push(time=push_time, impulse=imp)
    g.synchronize()
    assert g.step_log_count() == 0                                 # (create_initial_run never logs, and no log is enabled)
    return g


def run_chain(base, closed, K, read_back=True):
    """K one-step launches on a logging clone of `base`.  Returns the records, and per step the record the read-back entries give, the merit,
    the statistics row of instance 1 and the solve number; then the final snapshot"""
    dt, B = base.cfg['integrator_dt'], base.batch
    g = base.clone()
    g.step_log_enable(K)
    expected, merits, rows = [], [], []
    for i in range(K):
        t_init = i * dt + dt if closed else i * dt                   # the init_time handed to the solve (srbm_plant.hiph / srbm_fused.hiph)
        if read_back:
            node1 = g.trajectory_states()[:, 1, :].copy()
            pos_prev = g.eval_trajectory(t_init)[1]                 # the previous trajectory's foot locations at that time
        step(g, closed, i, 1)
        g.synchronize()
        info = g.debug_launch_info()
        assert info['steps'] == 1 and not info['queued'], info
        assert g.step_log_count() == i + 1
        if not read_back:
            continue
        st, err = g.status()
        e = np.zeros((B, host.STEP_LOG_DOUBLES))
        e[:, F['solve_number']] = g.status_accumulated()[:, 1:2]   # solves since creation: the 10 of the cold start + this chain's
        e[:, F['init_time']] = np.array([[tr.init_time] for tr in g.get_trajectory()])
        assert np.all(e[:, 1] == t_init) and np.all(e[:, 0] == 10 + i + 1)
        e[:, 2], e[:, 3], e[:, 4] = st, err, g.solve_flags()
        e[:, 5:7] = g.sizes()[:, :2]
        e[:, F['stats']] = g.stats()
        e[:, 15] = g.qp_cost()
        merit, merit_dd = g.merit()
        e[:, 16] = merit_dd
        e[:, F['state']] = g.plant_state() if closed else node1
        e[:, F['ee']] = pos_prev.reshape(B, 12)
        buf = io.StringIO()
        g.print_stat_line(buf, int(e[1, 0]), 1.25 + i, inst=1)
        force, _, contact = g.eval_trajectory(t_init)               # (last: it may raise error bits of its own)
        e[:, F['force']] = force.reshape(B, 12)
        e[:, F['in_contact']] = contact
        expected.append(e); merits.append(merit); rows.append(buf.getvalue())
    out = dict(records=g.step_log(), expected=np.array(expected), merit=np.array(merits), rows=rows, final=snapshot(g, closed))
    g.close()
    return out


def run_split(base, closed, split, log=True):
    g = base.clone()
    if log:
        g.step_log_enable(sum(split))
    first, infos = 0, []
    for k in split:
        step(g, closed, first, k)
        g.synchronize()
        infos.append(g.debug_launch_info())
        first += k
    out = dict(records=g.step_log() if log else None, final=snapshot(g, closed), infos=infos)
    g.close()
    return out


@pytest.fixture(scope='module')
def base_b():
    g = cold_start(load_config(), 4)
    yield g
    g.close()


@pytest.fixture(scope='module')
def chains(base_b):
    """the one-step chains of Config B, 4 instances x 6 steps, open and closed loop: computed once, read by several tests"""
    return {closed: run_chain(base_b, closed, 6) for closed in (False, True)}


@pytest.mark.parametrize('closed', [False, True], ids=['open_loop', 'closed_loop'])
def test_records_of_every_launch_form_equal_the_read_backs(base_b, chains, closed):
    """Config B, B = 4, K = 6, lower-start mode; closed loop with pushes at 2.5 dt on instances 0 and 1 and 4 sub-steps"""
    ch = chains[closed]
    rec = ch['records']
    assert rec.shape == (6, 4, 64)
    one = run_split(base_b, closed, (6,))
    two = run_split(base_b, closed, (2, 4))
    assert [i['kernel'] for i in one['infos'] + two['infos']] == ['srbm_rti_fused'] * 3        # a logged launch reports its unlogged twin
    same_bytes(one['records'], rec, 'one 6-step launch against the chain')
    same_bytes(two['records'], rec, 'the split (2, 4) against the chain')
    same_bytes(rec, ch['expected'], 'records against the read-backs of the one-step launches')
    same_bytes(host.step_log_merit(rec), ch['merit'], 'merit derived from the record against srbm_get_merit')
    assert not rec[:, :, 58:].any()                                                          # reserved
    # logging changes no result
    plain = run_split(base_b, closed, (6,), log=False)
    assert_bitwise(one['final'], plain['final'], 'logging 6-step launch against a non-logging one')
    assert_bitwise(two['final'], plain['final'], 'logging split against a non-logging launch')
    assert_bitwise(ch['final'], plain['final'], 'logging chain against a non-logging launch')
    # what the case covered
    assert np.all(rec[:, :, F['err']] == 0)
    flags = rec[:, :, F['in_contact']]
    print('step log closed=%d: solve flags %s, contact flags per step (instance 0) %s' %
          (closed, rec[:, :, 4].astype(int).tolist(), flags[:, 0].astype(int).tolist()))
    if not closed:
        assert (rec[:, :, F['solve_flags']] != 0).any()
    else:
        assert (rec[3, 0, F['state']] != rec[3, 2, F['state']]).any() and (rec[3, 1, F['state']] != rec[3, 2, F['state']]).any()
        # the push of instance 0 (0.4 on lin-mom x, in step 2) is in its record: a clone without pushes logs another state there, the same before
        g = base_b.clone(); g.plant_set_push(); g.step_log_enable(3); step(g, True, 0, 3); g.synchronize()
        calm = g.step_log(); g.close()
        same_bytes(calm[:2], rec[:2], 'before the push')
        assert abs((rec[2, 0, 20] - calm[2, 0, 20]) - 0.4) < 1e-12 and np.array_equal(calm[2, 2], rec[2, 2])
    assert np.isin(flags, (0, 1)).all() and flags.min() == 0 and flags.max() == 1
    # the contact flags move with the steps: the default schedule switches stance at t = 0.3, which the closed loop's init_time (dt .. 6 dt)
    # reaches in its sixth step and the open loop's (0 .. 5 dt) does not -- the case's two runs together show both patterns
    both = np.concatenate([chains[c]['records'][:, :, F['in_contact']] for c in (False, True)])
    assert any((both[s] != both[0]).any() for s in range(1, 12)), 'the contact flags never change over the steps of the case'


def test_step_queues_write_the_records_of_the_chain():
    """a batch of n_cu + 8 instances, 4 closed-loop steps: the multi-step launch runs on the step queues (srbm_rti_queued_logged)"""
    cfg = load_config()
    base = cold_start(cfg, chip_cu_count() + 8)
    ch = run_chain(base, True, 4, read_back=False)
    q = run_split(base, True, (4,))
    assert q['infos'][0]['kernel'] == 'srbm_rti_queued' and q['infos'][0]['queued'], q['infos']
    same_bytes(q['records'], ch['records'], 'queued 4-step launch against the chain')
    assert_bitwise(q['final'], ch['final'], 'queued launch against the chain')
    assert np.all(q['records'][:, :, F['solve_number']] == 11 + np.arange(4)[:, None, None])
    base.close()


def test_large_build_long_kernel_writes_the_records_of_the_chain():
    """N = 40 on the LARGE-capacity build: srbm_rti_fused_long_logged"""
    base = cold_start(load_config(num_nodes=40), 2, large=True)
    ch = run_chain(base, False, 3)
    one = run_split(base, False, (3,))
    assert one['infos'][0]['kernel'] == 'srbm_rti_fused_long', one['infos']
    same_bytes(one['records'], ch['records'], '3-step launch against the chain')
    same_bytes(ch['records'], ch['expected'], 'records against the read-backs')
    base.close()


def test_cursor_and_refusals(base_b):
    g = base_b.clone()
    assert g.step_log_count() == 0
    with pytest.raises(RuntimeError):
        g.step_log()                                               # no log enabled (a clone has logging off)
    g.step_log_enable(5)
    g.rti_advance(0, 3); g.synchronize()
    assert g.step_log_count() == 3
    before = snapshot(g, True)
    for call in (lambda: g.rti_advance(3, 3), lambda: g.closed_loop_advance(3, 3), lambda: g.rti_advance_unfused(3, 3)):
        with pytest.raises(RuntimeError, match='step log'):
            call()
    g.synchronize()
    assert g.step_log_count() == 3
    assert_bitwise(snapshot(g, True), before, 'after the refused calls')
    assert g.step_log(1, 2).shape == (2, 4, 64)
    for first, count in ((0, 4), (3, 1), (-1, 1), (4, 0), (1, -1)):
        with pytest.raises(RuntimeError):
            g.step_log(first, count)
    c = g.clone()                                                  # a clone of a logging batch: logging off
    c.rti_advance(3, 1); c.synchronize()
    assert c.step_log_count() == 0
    c.close()
    g.step_log_reset()
    assert g.step_log_count() == 0
    with pytest.raises(RuntimeError):
        g.step_log(0, 1)
    g.rti_advance_unfused(3, 2); g.synchronize()                   # one record per step of the unfused form, the buffer was kept
    assert g.step_log_count() == 2
    g.step_log_enable(0)
    with pytest.raises(RuntimeError):
        g.step_log(0, 0)
    g.rti_advance(5, 1); g.synchronize()                           # logging off: launches again without a log
    assert g.step_log_count() == 0
    g.close()


def test_unfused_steps_log_the_records_of_the_chain(base_b, chains):
    g = base_b.clone()
    g.step_log_enable(6)
    g.rti_advance_unfused(0, 6); g.synchronize()
    rec = g.step_log()
    g.close()
    # the unfused form makes no lower-start attempt (include/srbm_rti.h): its solves are not the chain's, its records are its own read-backs
    assert rec.shape == (6, 4, 64) and np.all(rec[:, :, 0] == 11 + np.arange(6)[:, None]) and np.all(rec[:, :, F['solve_flags']] == 0)
    same_bytes(rec[:, :, 1], chains[False]['records'][:, :, 1], 'init_time')


def test_get_real_time_update_logs_one_record(base_b):
    g = base_b.clone()
    g.step_log_enable(2)
    B = g.batch
    rng = np.random.default_rng(3)
    state = g.trajectory_states()[:, 1, :] + 0.0
    state[:, :3] += rng.uniform(-1e-3, 1e-3, (B, 3))
    t = np.full(B, 0.05); t[1] = 0.1
    ee = g.eval_trajectory(t)[1].reshape(B, 12)
    g.get_real_time_update(state, t, ee)
    assert g.step_log_count() == 1
    r = g.step_log()[0]
    st, err = g.status()
    e = np.zeros((B, 64))
    e[:, 0], e[:, 1], e[:, 2], e[:, 3], e[:, 4] = 11, t, st, err, g.solve_flags()
    e[:, 5:7] = g.sizes()[:, :2]
    e[:, F['stats']] = g.stats(); e[:, 15] = g.qp_cost(); e[:, 16] = g.merit()[1]
    e[:, F['state']] = state; e[:, F['ee']] = ee
    force, _, contact = g.eval_trajectory(t)
    e[:, F['force']] = force.reshape(B, 12); e[:, F['in_contact']] = contact
    same_bytes(r[None], e[None], 'srbm_get_real_time_update against its read-backs')
    g.close()


def test_device_copy_equals_the_host_copy(base_b):
    hip = C.CDLL('libamdhip64.so')
    g = base_b.clone()
    g.step_log_enable(4)
    g.closed_loop_advance(0, 4, SUBSTEPS, True)
    out = np.full((3, 4, 64), -7.0)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(out.nbytes)) == 0
    try:
        g.step_log_copy_dev(p.value, 1, 3)                         # queued behind the launch on the batch's stream: no synchronisation before it
        g.synchronize()
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes), 2) == 0      # hipMemcpyDeviceToHost
        with pytest.raises(RuntimeError):
            g.step_log_copy_dev(p.value, 2, 3)
    finally:
        hip.hipFree(p)
    same_bytes(out, g.step_log(1, 3), 'device copy against srbm_step_log_get')
    assert np.all(out[:, :, 0] == 12 + np.arange(3)[:, None])
    g.close()


@pytest.mark.parametrize('closed', [False, True], ids=['open_loop', 'closed_loop'])
def test_stat_lines_from_one_launch_equal_those_after_one_step_launches(base_b, chains, closed):
    one = run_split(base_b, closed, (6,))
    rows = []
    for i in range(6):
        buf = io.StringIO()
        host.stat_line_from_log(buf, one['records'][i, 1], 1.25 + i)
        rows.append(buf.getvalue())
    assert rows == chains[closed]['rows']
    assert len(set(rows)) == 6 and all(r.startswith('%d' % (11 + i)) for i, r in enumerate(rows))
