"""What a whole-controller rollout costs (srbm_controller_advance), by the protocol of dev_control_tick.py:
256 Config-B instances after the cold start, 200 ticks of 1 ms, an MPC update every 50 ticks, the variants in turn on fresh clones, three runs each;
medians and spreads.
  (a) entry      srbm_controller_advance, all ticks in one call (without and with a tick log: the difference is what the logged kernel adds)
  (b) chain      the loop driven from the host: srbm_control_tick_dev, srbm_wb_plant_step_dev, srbm_get_real_time_update_dev
  (c) plant      the plant-step kernel alone (srbm_wb_plant_step_dev, unlogged), 200 launches on the outputs of one tick
  (d) torque     srbm_controller_advance with the torque-driven plant (srbm_wb_plant_set_kind 1: PD 20 / 0.5, the configured torque bounds as
                 limits, the controller's bodies), logged, S = 1 and S = 4 sub-steps per tick; beside (a) this is what the plant kind costs.  And
                 its step kernel alone (srbm_wb_fd_step_dev, S = 1 and 4), as (c)
  (e) ground     (d) with a compliant ground set (srbm_wb_plant_set_ground: k_n 2e4, d_n 100, mu 0.7, k_t 1e4, d_t 50, the plane 3 mm above each
                 instance's lowest foot at the start), logged, S = 1 and 4; beside (d) this is what the ground costs.  And its step kernel alone
                 (srbm_wb_ground_step_dev, S = 1 and 4), as (c)
  (t) terrain    (e) at S = 4 with a terrain of 8 patches set (srbm_wb_plant_set_terrain: the ground's plane as patch 0 and over it seven strips 0.1 m
                 wide in x, sloped by +-1 % about their centre lines, friction 0.7 and 0.4 in turn), logged; beside (e) this is what the terrain
                 costs.  And its step kernel alone, S = 1 and 4, interleaved with the ground step kernel alone on the same inputs.  Skipped, with
                 a note in the output, on a library that has no terrain (a parent's build run from a copy of its tree)
  (f) feedback   (e) at S = 4 with contact feedback on (srbm_controller_set_contact_feedback: one small launch per MPC update); beside (e) this is
                 what the feedback costs -- per update: the difference times ticks_per_update
  (g) gait       (e) at S = 4 through srbm_gait_controller_advance with gait_opt_freq 5, feedback off, 250 ticks so that the updates are three plain
                 ones, one with gradient and LP (run 4) and one line search (run 5); ms per tick over those 250 ticks
  (l) latency    (a) logged with an MPC computation latency set (srbm_controller_set_latency): 0 everywhere; a constant 20 ms (one launch of the
                 publish kernel per update); per_iteration 1 ms with base 0 (the kernel launched before every tick of a period: nothing bounds
                 the solve's iterations below the forced tick); each beside (a) logged of the same run, with the
                 iterations of the whole-body QP per tick and of the IPM per update (a step log is on): trajectories in force later make other
                 rollouts, whose ticks and updates cost what their solves take.  And the publish kernel alone
                 (srbm_controller_publish_dev), 200 launches in which every instance is published (a new update number each, forced) and 200 in
                 which none is (the same update number again); and (b) with latency 0 set and the publish kernel launched before every tick: the same
                 rollout as (b), so the difference is what a launch per tick costs.  Skipped, with a note, on a library without the setting
  (s) sensors    (a) logged with sensors set (srbm_controller_set_sensors): the transparent model, whose rollout is (a)'s, so the difference is what the
                 measure kernel's launch per tick costs; everything on (mocap every 5 ticks one sample late, pose noise, finite-difference velocity,
                 gyro noise and bias, joint noise, both filters), another rollout, with the iterations of its whole-body QP; and the measure kernel
                 alone (srbm_controller_measure_dev), 200 launches with everything on.  Skipped, with a note, on a library without the setting
  (j) joints     (e) at S = 4 with a joint model set (srbm_wb_plant_set_joints: the A1's damping, armature, dry friction, ranges from
                 tests/golden/a1_joint_model.json, a stiction band of 0.1 rad/s, a motor time constant of 2 ms, stops of 200 N m/rad and 2 N m s/rad),
                 logged, with the model's record; beside (e) this is what the joint model costs.  And its ground step kernel alone, S = 1 and 4,
                 interleaved with the ground step kernel alone on the same inputs.  Skipped, with a note, on a library without the setting
  (w) wrenches   (e) at S = 4 with a wrench schedule set (srbm_wb_plant_set_wrenches), logged, with the schedule's record: eight events that never act
                 (beside (e): the event load and the activity test); one event always active (5 N on the trunk, off its origin); eight always
                 active (1.5 N each on eight bodies, world and body frames in turn, with torques) -- the last two are other rollouts.  And the
                 schedule's ground step kernel alone with each of the three, S = 1 and 4, interleaved with the ground step kernel alone on the same
                 inputs.  Skipped, with a note, on a library without the setting
  (m) commands   with --commands, these rows ALONE (the others are skipped): (a) logged, and (a) logged with a command schedule set
                 (srbm_controller_set_commands): one event whose t0 lies beyond the rollout (the schedule never acts: one launch per update that
                 returns on its test); one event in force that holds the cold start's target; a relative walk at 0.3 m/s with a lead of 0.1 s
                 (another rollout), each with the record's update count and largest distance.  On a library without the setting (a parent's build
                 run from a copy of its tree) the logged entry alone, with a note: the parent's figure for the same rollout
Every launch is under a time limit of its own (an alarm re-armed per call: a launch or a wait that does not return ends the process).
Prints one JSON line."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srbm_loader import host
from srbm_loader.control_tick import ControlTick
from srbm_loader.controller_rollout import (ControllerRollout, TICK_LOG_FIELDS, TORQUE_PLANT_LOG_FIELDS, GROUND_PLANT_LOG_FIELDS, FLAG_COAST, FLAG_BREAKDOWN,
                                            PLANT_TORQUE_DRIVEN, decode_ground_word)
from srbm_loader.workloads import config_b_instance, instances

F = dict(TICK_LOG_FIELDS, **TORQUE_PLANT_LOG_FIELDS)
G = dict(TICK_LOG_FIELDS, **GROUND_PLANT_LOG_FIELDS)
B, TICKS, TPU, DT, LIMIT_S = 256, 200, 50, 1e-3, 60.0
COMMANDS = '--commands' in sys.argv[1:]
_ARGS = [a for a in sys.argv[1:] if a != '--commands']
RUNS = int(_ARGS[0]) if _ARGS else 3
GAIT_TICKS, GAIT_FREQ = 250, 5


def main():
    import torch
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    cfg = host.load_config('a1_configuration')
    states, ees = instances(cfg, config_b_instance, B)
    signal.setitimer(signal.ITIMER_REAL, 300.0)
    base = host.BatchMPC.cold_start(cfg, states, ees)
    q_init = np.tile(np.array(cfg['init_config'], float), (B, 1))
    q0, v0, _, st = base.clone().get_targets_from_traj(0.0, q_init)          # the plant starts on the targets of tick 0
    res = {'entry': [], 'entry_logged': [], 'chain': [], 'plant': [], 'torque_s1_logged': [], 'torque_s4_logged': [], 'fd_step_s1': [], 'fd_step_s4': [],
           'ground_s1_logged': [], 'ground_s4_logged': [], 'ground_step_s1': [], 'ground_step_s4': [], 'ground_s4_feedback_logged': [],
           'ground_s4_gait_f5_logged': []}
    has_terrain = hasattr(ControllerRollout, 'set_terrain')
    has_latency = hasattr(ControllerRollout, 'set_latency')
    if has_latency:
        res.update({'latency_0': [], 'latency_20ms': [], 'latency_per_iteration': [], 'chain_latency_0_every_tick': [], 'publish_all': [], 'publish_none': []})
    if has_terrain:
        res.update({'terrain_s4_logged': [], 'terrain_step_s1': [], 'terrain_step_s4': []})
    has_sensors = hasattr(ControllerRollout, 'set_sensors')
    if has_sensors:
        from srbm_loader import sensors
        res.update({'sensors_transparent': [], 'sensors_all': [], 'measure': []})
        sens_transparent = sensors.record()
        sens_all = sensors.record(mocap_ticks=5, mocap_delay=1, sigma_p=1e-3, sigma_r=2e-3, velocity_source=1, sigma_w=0.01, gyro_bias=(0.01, -0.01, 0.005),
                                  sigma_qj=1e-3, sigma_vj=0.05, lpf_base=sensors.lpf_x(40.0, DT), lpf_joints=sensors.lpf_x(100.0, DT))
    has_joints = hasattr(ControllerRollout, 'set_joints')
    if has_joints:
        from srbm_loader import joints as joint_model
        res.update({'joints_s4_logged': [], 'joint_ground_step_s1': [], 'joint_ground_step_s4': []})
        a1_joints, _ = joint_model.a1_model(json.load(open(os.path.join(ROOT, 'tests', 'golden', 'a1_joint_model.json'))), 0.1, 2e-3)
        a1_stops = (200.0, 2.0)
    has_wrenches = hasattr(ControllerRollout, 'set_wrenches')
    if has_wrenches:
        from srbm_loader import wrenches as wr
        schedules = {'never': [wr.event(1e3, np.inf, i) for i in range(8)],
                     'one': [wr.event(0.0, np.inf, 'trunk', point=(0.05, 0.0, 0.02), force=(0.0, 5.0, 0.0))],
                     'eight': [wr.event(0.0, np.inf, 1 + (5 * i) % 12 if i else 0, point=(0.02, 0.01, -0.03), force=(1.5 * (-1) ** i, 0.5, -0.5),
                                        torque=(0.0, 0.05, 0.02), frame='body' if i % 2 else 'world') for i in range(8)]}
        schedules = {k: wr.schedule(B, [v]) for k, v in schedules.items()}
        for k in schedules:
            res.update({'wrench_%s_s4_logged' % k: [], 'wrench_%s_ground_step_s1' % k: [], 'wrench_%s_ground_step_s4' % k: []})
    ground = terrain = None
    kp, kd, lim = np.full(12, 20.0), np.full(12, 0.5), np.asarray(cfg['torque_bounds'], float)
    info = {}
    f64 = dict(dtype=torch.float64, device='cuda')

    def fresh(tick_log=0):
        g = base.clone()
        R = ControllerRollout(g)
        R.reset(q_init); R.set_state(q0, v0)
        if tick_log:
            R.tick_log_enable(tick_log)
        return g, R

    def timed(g, fn):
        g.synchronize()
        tb = time.perf_counter()
        fn()
        g.synchronize()
        return 1e3 * (time.perf_counter() - tb) / TICKS

    if COMMANDS:          # --commands: rows (m) alone
        has_commands = hasattr(ControllerRollout, 'set_commands')
        rows = {'entry_logged': None}
        if has_commands:
            from srbm_loader import commands as cmd
            _, des = host._tracking_cost(cfg)
            rel = des.copy(); rel[:2] = 0.0
            rows.update({'commands_never': cmd.stack([[cmd.walk(1e3, 0.3, 0.0, cfg['mass'], rel, lead=0.1)]], batch=B),
                         'commands_hold': cmd.stack([[cmd.hold(0.0, des)]], batch=B),
                         'commands_walk': cmd.stack([[cmd.walk(0.0, 0.3, 0.0, cfg['mass'], rel, lead=0.1)]], batch=B)})
        else:
            info['commands'] = 'this library has no command schedule: rows (m) are the logged entry alone'
        res = {k: [] for k in rows}
        for run in range(RUNS):
            for name, schedule in rows.items():
                g, R = fresh(TICKS + 3)
                if schedule is not None:
                    R.set_commands(schedule)
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                R.advance(0, 3, TPU, DT)
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
                log = R.tick_log()
                info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), mean_qp_iterations=float(log[:, :, F['qp_iters']].mean()),
                                  base_x_moved_mean=float((R.state()[0][:, 0] - q0[:, 0]).mean()))
                if schedule is not None:
                    crec = R.command_record()
                    info[name].update(updates_with_an_event=int(crec[:, 0].sum()), max_distance=float(crec[:, 6].max()))
        signal.setitimer(signal.ITIMER_REAL, 0)
        print(json.dumps(dict(batch=B, ticks=TICKS, ticks_per_update=TPU, tick_dt=DT, runs=RUNS, ms_per_tick_runs=res,
                              ms_per_tick_median={k: float(np.median(v)) for k, v in res.items()},
                              spread_ms={k: float(max(v) - min(v)) for k, v in res.items()}, **info)))
        return
    for run in range(RUNS):
        for name, tl in (('entry', 0), ('entry_logged', TICKS + 3)):
            g, R = fresh(tl)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)                                          # warm-up: three ticks
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            if tl:
                log = R.tick_log()
                info['coasted_ticks'] = int(((log[:, :, F['flags']].astype(int) & FLAG_COAST) != 0).sum())
                info['targets_not_ok'] = int((log[:, :, F['targets_status']] != 0).sum())
                info['base_height_range'] = [float(log[:, :, 8].min()), float(log[:, :, 8].max())]
                info['mean_qp_iterations'] = float(log[:, :, F['qp_iters']].mean())
                info['slowest_qp_iterations_mean'] = float(log[:, :, F['qp_iters']].max(axis=1).mean())
            info['finite_' + name] = bool(np.all(np.isfinite(R.state()[0])))
        # (d) the torque-driven plant
        for S in (1, 4):
            name = 'torque_s%d_logged' % S
            g, R = fresh(TICKS + 3)
            R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log = R.tick_log()
            info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())],
                              zero_action_ticks=int((log[:, :, F['qp_status']] > 1).sum()), mean_qp_iterations=float(log[:, :, F['qp_iters']].mean()),
                              breakdown_ticks=int(((log[:, :, F['flags']].astype(int) & FLAG_BREAKDOWN) != 0).sum()),
                              clamped_ticks=int((log[:, :, F['clamped_joints']] > 0).sum()), min_stance_fz=float(log[:, :, F['min_stance_fz']].min()),
                              pulling_ticks=int((log[:, :, F['min_stance_fz']] < 0).sum()),
                              median_accel_mismatch=float(np.median(log[:, :, F['accel_mismatch']])), max_accel_mismatch=float(log[:, :, F['accel_mismatch']].max()))
            if ground is None:          # the plane 3 mm above each instance's lowest foot of the first tick
                ground = np.zeros((B, 8))
                ground[:, 0] = log[0][:, F['foot_heights']].min(axis=1) + 0.003
                ground[:, 1:6] = [2e4, 100.0, 0.7, 1e4, 50.0]
        # (e) ... on its ground
        for S in (1, 4):
            name = 'ground_s%d_logged' % S
            g, R = fresh(TICKS + 3)
            R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
            R.set_ground(ground)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log = R.tick_log()
            word = decode_ground_word(log[:, :, G['ground_word']])
            info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())],
                              zero_action_ticks=int((log[:, :, G['qp_status']] > 1).sum()), mean_qp_iterations=float(log[:, :, G['qp_iters']].mean()),
                              slowest_qp_iterations_mean=float(log[:, :, G['qp_iters']].max(axis=1).mean()),
                              breakdown_ticks=int(((log[:, :, G['flags']].astype(int) & FLAG_BREAKDOWN) != 0).sum()),
                              clamped_ticks=int((log[:, :, G['clamped_joints']] > 0).sum()),
                              min_planned_stance_fz=float(log[:, :, G['min_planned_stance_fz']].min()),
                              feet_in_contact_mean=float(word['in_contact'].sum(axis=-1).mean()), slipping_feet_mean=float(word['slipping'].sum(axis=-1).mean()),
                              feet_off_the_plan_mean=float(word['plan_differs'].sum(axis=-1).mean()),
                              median_accel_mismatch=float(np.median(log[:, :, G['accel_mismatch']])))
        # (t) ... with a terrain of 8 patches
        if has_terrain:
            if terrain is None:
                terrain = np.zeros((B, 8, 8))
                x0 = q0[:, 0] - 0.35
                for b in range(B):
                    terrain[b, 0] = [-np.inf, np.inf, -np.inf, np.inf, ground[b, 0], 0.0, 0.0, 0.7]
                    for t in range(1, 8):
                        lo, gx = x0[b] + 0.1 * (t - 1), 0.01 * (-1) ** t
                        terrain[b, t] = [lo, lo + 0.1, -np.inf, np.inf, ground[b, 0] - gx * (lo + 0.05), gx, 0.0, 0.7 if t % 2 else 0.4]
            g, R = fresh(TICKS + 3)
            R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 4)
            R.set_ground(ground)
            R.set_terrain(terrain)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res['terrain_s4_logged'].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log = R.tick_log()
            word = decode_ground_word(log[:, :, G['ground_word']])
            info['terrain_s4_logged'] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())],
                                             zero_action_ticks=int((log[:, :, G['qp_status']] > 1).sum()), mean_qp_iterations=float(log[:, :, G['qp_iters']].mean()),
                              slowest_qp_iterations_mean=float(log[:, :, G['qp_iters']].max(axis=1).mean()),
                                             clamped_ticks=int((log[:, :, G['clamped_joints']] > 0).sum()), patches_stood_on=sorted(set(R.contact_state()[:, :, 0].ravel().tolist())),
                                             breakdown_ticks=int(((log[:, :, G['flags']].astype(int) & FLAG_BREAKDOWN) != 0).sum()),
                                             min_planned_stance_normal_force=float(log[:, :, G['min_planned_stance_fz']].min()),
                                             feet_in_contact_mean=float(word['in_contact'].sum(axis=-1).mean()),
                                             slipping_feet_mean=float(word['slipping'].sum(axis=-1).mean()),
                                             feet_off_the_plan_mean=float(word['plan_differs'].sum(axis=-1).mean()))
        # (j) ... with the A1's joint model
        if has_joints:
            g, R = fresh(TICKS + 3)
            R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 4)
            R.set_ground(ground)
            R.set_joints(a1_joints, a1_stops)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res['joints_s4_logged'].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log, jrec = R.tick_log(), R.joint_record()
            info['joints_s4_logged'] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())],
                                            zero_action_ticks=int((log[:, :, G['qp_status']] > 1).sum()), mean_qp_iterations=float(log[:, :, G['qp_iters']].mean()),
                                            slowest_qp_iterations_mean=float(log[:, :, G['qp_iters']].max(axis=1).mean()),
                                            breakdown_ticks=int(((log[:, :, G['flags']].astype(int) & FLAG_BREAKDOWN) != 0).sum()),
                                            clamped_ticks=int((log[:, :, G['clamped_joints']] > 0).sum()), substeps=int(jrec[:, 0].sum()),
                                            substeps_beyond_a_range=int(jrec[:, 1].sum()), max_excursion=float(jrec[:, 2].max()),
                                            max_friction_torque=float(jrec[:, 3].max()), max_motor_lag=float(jrec[:, 4].max()))
        # (w) ... with a wrench schedule: never active, one event always active, eight always active
        for k, W in schedules.items() if has_wrenches else ():
            name = 'wrench_%s_s4_logged' % k
            g, R = fresh(TICKS + 3)
            R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 4)
            R.set_ground(ground)
            R.set_wrenches(W)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log, wrec = R.tick_log(), R.wrench_record()
            info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())],
                              zero_action_ticks=int((log[:, :, G['qp_status']] > 1).sum()), mean_qp_iterations=float(log[:, :, G['qp_iters']].mean()),
                              slowest_qp_iterations_mean=float(log[:, :, G['qp_iters']].max(axis=1).mean()),
                              breakdown_ticks=int(((log[:, :, G['flags']].astype(int) & FLAG_BREAKDOWN) != 0).sum()),
                              ticks_with_an_event=int(((log[:, :, G['flags']].astype(int) & 16) != 0).sum()), substeps=int(wrec[:, 0].sum()),
                              substeps_active=int(wrec[:, 1].sum()), max_generalized_force=float(wrec[:, 3].max()))
        # (f) ... with contact feedback on
        g, R = fresh(TICKS + 3)
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 4)
        R.set_ground(ground)
        R.set_contact_feedback(True)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        R.advance(0, 3, TPU, DT)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        res['ground_s4_feedback_logged'].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
        fb = R.contact_feedback()
        info['ground_s4_feedback_logged'] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), touch_downs_moved=int(fb[:, :, 0].sum()),
                                                 instances_with_a_move=int((fb[:, :, 0].sum(axis=1) > 0).sum()),
                                                 error_bits=int(np.bitwise_or.reduce(g.status_accumulated()[:, 0])))
        # (g) ... and with the gait step in the updates
        g, R = fresh(GAIT_TICKS + 3)
        R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, 4)
        R.set_ground(ground)
        gait = host.BatchGaitOptimizer(g)
        g.step_log_enable(GAIT_TICKS // TPU + 1)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        R.advance(0, 3, TPU, DT, gait=gait, gait_opt_freq=GAIT_FREQ)
        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
        res['ground_s4_gait_f5_logged'].append(timed(g, lambda: R.advance(3, GAIT_TICKS, TPU, DT, gait=gait, gait_opt_freq=GAIT_FREQ)) * TICKS / GAIT_TICKS)
        steps = g.step_log()
        info['ground_s4_gait_f5_logged'] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), ticks=GAIT_TICKS, run_kinds=[int(x) for x in steps[:, 0, 58]],
                                                ready_after_the_gradient_run=int(steps[:, :, 59].max(axis=0).sum()),
                                                searched_in_the_line_search=int((steps[:, :, 58] == 2).sum()))
        gait.close()
        # (l) the logged entry with a latency set
        for name, lat in (('latency_0', (0.0, 0.0)), ('latency_20ms', (0.02, 0.0)), ('latency_per_iteration', (0.0, 1e-3))) if has_latency else ():
            g, R = fresh(TICKS + 3)
            R.set_latency(*lat)
            g.step_log_enable(TICKS // TPU + 1)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            rec, log, steps = R.latency_record(), R.tick_log(), g.step_log()
            info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), mean_qp_iterations=float(log[:, :, F['qp_iters']].mean()),
                              slowest_qp_iterations_mean=float(log[:, :, F['qp_iters']].max(axis=1).mean()),
                              updates=int(steps.shape[0]), mean_ipm_iterations=float(steps[:, :, 11].mean()),
                              slowest_ipm_iterations_mean=float(steps[:, :, 11].max(axis=1).mean()), publications=int(rec[:, 1].sum()), overruns=int(rec[:, 2].sum()),
                              max_latency=float(rec[:, 6].max()), mean_age_at_publication=float((rec[:, 7] / np.maximum(rec[:, 1], 1)).mean()))
        # (s) the logged entry with sensors set: the transparent model, and everything on
        for name, sens in (('sensors_transparent', sens_transparent), ('sensors_all', sens_all)) if has_sensors else ():
            g, R = fresh(TICKS + 3)
            R.set_sensors(sens, np.arange(B))
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            R.advance(0, 3, TPU, DT)
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res[name].append(timed(g, lambda: R.advance(3, TICKS, TPU, DT)))
            log, srec = R.tick_log(), R.sensor_record()
            info[name] = dict(finite=bool(np.all(np.isfinite(R.state()[0]))), mean_qp_iterations=float(log[:, :, F['qp_iters']].mean()),
                              slowest_qp_iterations_mean=float(log[:, :, F['qp_iters']].max(axis=1).mean()),
                              coasted_ticks=int(((log[:, :, F['flags']].astype(int) & FLAG_COAST) != 0).sum()),
                              base_height_range=[float(log[:, :, 8].min()), float(log[:, :, 8].max())], samples=int(srec[:, 1].sum()),
                              max_errors=[float(x) for x in srec[:, 2:].max(axis=0)])
        # (b) the same loop from the host, on torch's buffers, on the batch's stream
        g, R = fresh()
        T = ControlTick(g)
        with torch.cuda.stream(torch.cuda.ExternalStream(g.stream())):
            q_d, v_d, t_d = torch.tensor(q0, **f64), torch.tensor(v0, **f64), torch.zeros(B, **f64)
            ctl_d, sol_d, x_d, ee_d = torch.zeros((B, 36), **f64), torch.zeros((B, 30), **f64), torch.zeros((B, 13), **f64), torch.zeros((B, 12), **f64)
            st_d, con_d = torch.zeros((B, 2), dtype=torch.int32, device='cuda'), torch.zeros((B, 4), dtype=torch.int32, device='cuda')

            def chain(first, n):
                for k in range(first, first + n):
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    t_d.fill_(k * DT)
                    T.tick_dev(q_d.data_ptr(), v_d.data_ptr(), t_d.data_ptr(), ctl_d.data_ptr(), sol_d.data_ptr(), st_d.data_ptr(), None, None,
                               con_d.data_ptr(), x_d.data_ptr(), ee_d.data_ptr())
                    R.plant_step_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), sol_d.data_ptr(), st_d.data_ptr())
                    if k > 0 and k % TPU == 0:
                        g.get_real_time_update_dev(x_d.data_ptr(), t_d.data_ptr(), ee_d.data_ptr())
            chain(0, 3)
            res['chain'].append(timed(g, lambda: chain(3, TICKS)))
            info['finite_chain'] = bool(torch.isfinite(q_d).all().item())

            # (c) the plant-step kernel alone
            def plant():
                for k in range(TICKS):
                    R.plant_step_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), sol_d.data_ptr(), st_d.data_ptr())
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            plant()
            signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
            res['plant'].append(timed(g, plant))

            # ... and the torque-driven step kernel alone, on the same outputs
            for S in (1, 4):
                R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
                q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64))

                def fd_step():
                    for k in range(TICKS):
                        R.fd_step_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), ctl_d.data_ptr(), con_d.data_ptr(), st_d.data_ptr())
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                fd_step()
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                res['fd_step_s%d' % S].append(timed(g, fd_step))

            # ... and the ground step kernel alone
            R.set_ground(ground)
            cs_d = torch.zeros((B, 12), **f64)
            for S in (1, 4):
                R.set_plant(PLANT_TORQUE_DRIVEN, kp, kd, lim, S)
                q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64)); cs_d.zero_()

                def ground_step():
                    for k in range(TICKS):
                        R.ground_step_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), cs_d.data_ptr(), ctl_d.data_ptr(), st_d.data_ptr())
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                ground_step()
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                res['ground_step_s%d' % S].append(timed(g, ground_step))
                if has_terrain:         # ... and the terrain step kernel alone: the same entry with the terrain in force, from the same start
                    R.set_terrain(terrain)
                    q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64)); cs_d.zero_()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    ground_step()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    res['terrain_step_s%d' % S].append(timed(g, ground_step))
                    R.set_terrain(None)
                if has_joints:          # ... and the joint model's ground step kernel alone: the same entry with the model in force, from the same start
                    R.set_joints(a1_joints, a1_stops)
                    q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64)); cs_d.zero_()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    ground_step()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    res['joint_ground_step_s%d' % S].append(timed(g, ground_step))
                    R.set_joints(None)
                for k, W in schedules.items() if has_wrenches else ():          # ... and the schedule's ground step kernel alone, likewise
                    R.set_wrenches(W)
                    q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64)); cs_d.zero_()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    ground_step()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    res['wrench_%s_ground_step_s%d' % (k, S)].append(timed(g, ground_step))
                    R.set_wrenches(None)
            # ... and the publish kernel alone: every instance published, no instance published
            if has_latency:
                R.set_latency(0.0)
                counter = [0]

                def publish_all():
                    for k in range(TICKS):
                        counter[0] += 1
                        R.publish_dev(t_d.data_ptr(), counter[0], 0.0, 1)

                def publish_none():
                    for k in range(TICKS):
                        R.publish_dev(t_d.data_ptr(), counter[0], 0.0, 1)
                for name, fn in (('publish_all', publish_all), ('publish_none', publish_none)):
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    fn()
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    res[name].append(timed(g, fn))
                info['publish_all_publications'] = int(R.latency_record()[:, 1].sum())
                R.set_latency(None)
            # ... and the measure kernel alone, everything on, on the same true state every launch
            if has_sensors:
                R.set_sensors(sens_all, np.arange(B))
                q_d.copy_(torch.tensor(q0, **f64)); v_d.copy_(torch.tensor(v0, **f64))
                qm_d, vm_d = torch.zeros((B, 19), **f64), torch.zeros((B, 18), **f64)

                def measure():
                    for k in range(TICKS):
                        R.measure_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), qm_d.data_ptr(), vm_d.data_ptr())
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                measure()
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                res['measure'].append(timed(g, measure))
                info['measure_ticks'] = int(R.sensor_record()[:, 0].sum())
                R.set_sensors(None)
        # ... and what a launch before EVERY tick costs in a rollout that is otherwise (b): the chain with latency 0 set, the publish kernel launched before
        # every tick (it publishes before the tick after an update and returns on its decision before every other one)
        if has_latency:
            g, R = fresh()
            R.set_latency(0.0)
            T = ControlTick(g)
            with torch.cuda.stream(torch.cuda.ExternalStream(g.stream())):
                q_d, v_d, t_d = torch.tensor(q0, **f64), torch.tensor(v0, **f64), torch.zeros(B, **f64)
                ctl_d, sol_d, x_d, ee_d = torch.zeros((B, 36), **f64), torch.zeros((B, 30), **f64), torch.zeros((B, 13), **f64), torch.zeros((B, 12), **f64)
                st_d, con_d = torch.zeros((B, 2), dtype=torch.int32, device='cuda'), torch.zeros((B, 4), dtype=torch.int32, device='cuda')

                def chain_published(first, n):
                    for k in range(first, first + n):
                        signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                        t_d.fill_(k * DT)
                        e = (k - 1) // TPU if k >= 1 else 0
                        R.publish_dev(t_d.data_ptr(), e, (e * TPU) * DT, int(k % TPU == 0 and e >= 1))
                        T.tick_dev(q_d.data_ptr(), v_d.data_ptr(), t_d.data_ptr(), ctl_d.data_ptr(), sol_d.data_ptr(), st_d.data_ptr(), None, None,
                                   con_d.data_ptr(), x_d.data_ptr(), ee_d.data_ptr())
                        R.plant_step_dev(k, DT, q_d.data_ptr(), v_d.data_ptr(), sol_d.data_ptr(), st_d.data_ptr())
                        if k > 0 and k % TPU == 0:
                            g.get_real_time_update_dev(x_d.data_ptr(), t_d.data_ptr(), ee_d.data_ptr())
                chain_published(0, 3)
                res['chain_latency_0_every_tick'].append(timed(g, lambda: chain_published(3, TICKS)))
                info['chain_latency_0_publications'] = int(R.latency_record()[:, 1].sum())
    signal.setitimer(signal.ITIMER_REAL, 0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    if not has_terrain:
        info['terrain'] = 'this library has no terrain: rows (t) skipped'
    if not has_latency:
        info['latency'] = 'this library has no latency setting: rows (l) skipped'
    if not has_joints:
        info['joints'] = 'this library has no joint model: rows (j) skipped'
    if not has_wrenches:
        info['wrenches'] = 'this library has no wrench schedule: rows (w) skipped'
    if not has_sensors:
        info['sensors'] = 'this library has no sensor model: rows (s) skipped'
    print(json.dumps(dict(batch=B, ticks=TICKS, ticks_per_update=TPU, tick_dt=DT, runs=RUNS, ms_per_tick_runs=res, ms_per_tick_median=med,
                          spread_ms={k: float(max(v) - min(v)) for k, v in res.items()}, **info)))


if __name__ == '__main__':
    main()
