"""Whole-controller rollouts (include/srbm_rti.h: srbm_controller_advance, srbm_wb_plant_*, srbm_tick_log_*): the loop of the reference's top-level
program (test/simulation_mpc.cpp:186-215) for every instance of a host.BatchMPC -- MPCController::ComputeControlAction every tick, an MPC update
every `ticks_per_update` ticks, and between them a whole-body plant: by default the one that integrates the accelerations of the whole-body QP
(it has no ground and no joint PD loop: the header says what that means), or, after set_plant(1, ...), the torque-driven one -- the constrained
forward dynamics of the plant's own bodies under the returned torques, the joint PD loop and the torque limits.  With a ground under that plant
(set_ground) the MPC update can be the reference's MPCUpdate in full: set_contact_feedback(True) runs MPC::AdjustForCurrentContacts on the ground's
contact state before every update, and advance(..., gait=, gait_opt_freq=) branches every update into line search / update + gradient + LP / plain
update (srbm_gait_controller_advance).  Without a ground nothing measures a contact, and there is no AdjustForCurrentContacts.
A module of its own beside host.py, as control_tick.py and mpc_period.py are: it calls through the library `host.declare` has typed, and
tests/test_abi_prototypes.py keeps the method list of host.BatchMPC as it stands.

    R = ControllerRollout(mpc)            mpc: a BatchMPC with leg kinematics and a whole-body model, after its cold start
    R.reset(q_des)                        the IK guess of the first tick (srbm_control_tick_reset)
    R.set_state(q, v)                     the plant's (q, v)
    mpc.plant_set_push(time, impulse)     optional: one push per instance
    R.set_plant(1, kp, kd, limit, 4)      optional: the torque-driven plant, 4 sub-steps per tick; R.set_plant_bodies(...): its own bodies
    R.set_ground(ground)                  optional, with set_plant(1, ...): a compliant ground [batch][8] under the torque-driven plant's feet
    R.set_terrain([terrain_patch(gx=0.1, mu=0.6), terrain_patch(x=(0.5, 1.0), gx=0.1, mu=0.1)])
                                          optional, with a ground: sloped patches with a friction coefficient each in place of its plane
    R.tick_log_enable(200)                optional: one record per tick and instance
    R.set_contact_feedback(True)          optional, with a ground: early touch-downs re-time the plan before every MPC update
    R.advance(0, 200, 50, 1e-3)           200 ticks of 1 ms, an MPC update every 50; asynchronous
    R.advance(0, 200, 50, 1e-3, gait=go, gait_opt_freq=5)      the same with the gait step of host.BatchGaitOptimizer `go` in the updates
    R.set_latency(0.02)                   optional: every update comes into force 20 ms after it started, not at the next tick; per instance:
                                          R.set_latency(base[batch], per_iteration) -- base + per_iteration * (IPM iterations of the solve)
    R.set_sensors(sens, seed)             optional: the ticks read a measurement of (q, v) -- mocap rate and delay, noise, gyro bias, low-pass filters --
                                          sens[batch][16] from srbm_loader.sensors.record(...), one 64-bit seed per instance
    R.set_joints(joints, stops)           optional, with set_plant(1, ...): a joint model -- damping, armature, dry friction, range stops, motor lag --
                                          joints[batch][12][8] from srbm_loader.joints.record(...) or joints.a1_model(), stops = (k_l, d_l)
    js = R.joint_state(); jrec = R.joint_record()
    R.set_wrenches(wrenches.schedule(batch, [[wrenches.event(0.5, 0.15, 'trunk', force=(0, 60, 0))]]))
                                          optional, with set_plant(1, ...): timed external forces and torques on any body (srbm_loader.wrenches)
    wrec = R.wrench_record()
    R.set_commands(commands.stack([[commands.hold(0.0, des12), commands.walk(0.5, 0.3, 0.0, mass, des12)]]))
                                          optional: the tracking target over time (srbm_loader.commands); crec = R.command_record()
    q, v = R.state(); log = R.tick_log(); pub = R.latency_record(); qm, vm = R.measured(); srec = R.sensor_record()"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

TICK_LOG_DOUBLES = 64
# one record of the tick log: field name -> slice of its TICK_LOG_DOUBLES doubles (include/srbm_rti.h); [57, 64) is 0 with the QP-acceleration plant
TICK_LOG_FIELDS = dict(tick=0, time=1, targets_status=2, qp_status=3, qp_iters=4, flags=5, base_pose=slice(6, 13), base_twist=slice(13, 19),
                       torques=slice(19, 31), contact_forces=slice(31, 43), contact=slice(43, 47), foot_heights=slice(47, 51), base_accel=slice(51, 57))
# ... and what the torque-driven plant writes into [57, 63) (field 63 stays 0): 58..62 are of the last sub-step of the tick
TORQUE_PLANT_LOG_FIELDS = dict(plant_kind=57, clamped_joints=58, torque_deviation=59, min_stance_fz=60, accel_mismatch=61, force_mismatch=62)
# ... and what it writes with a ground set (set_ground): 57..59 as above, 60..63 of the ground; 58..63 are of the last sub-step of the tick
GROUND_PLANT_LOG_FIELDS = dict(plant_kind=57, clamped_joints=58, torque_deviation=59, min_planned_stance_fz=60, accel_mismatch=61, force_mismatch=62,
                               ground_word=63)
GROUND_WORD_OFFSET = 4096
GROUND_DOUBLES, CONTACT_STATE_DOUBLES = 8, 12
TERRAIN_PATCHES, TERRAIN_DOUBLES = 8, 8      # host.TERRAIN_PATCHES, host.TERRAIN_DOUBLES: the most patches per instance, the doubles of a patch
CONTACT_FEEDBACK_DOUBLES = 8        # the feedback record of an instance: per foot {touch-downs moved, time of the last move (-1: none)}
FLAG_PUSH, FLAG_UPDATE, FLAG_COAST, FLAG_BREAKDOWN = 1, 2, 4, 8
LATENCY_RECORD_DOUBLES = 8          # the latency record of an instance (set_latency), field name -> index
LATENCY_RECORD_FIELDS = dict(update_in_force=0, publications=1, overruns=2, last_publication_time=3, t_start_in_force=4, last_latency=5, max_latency=6,
                             age_sum=7)
PLANT_QP_ACCELERATION, PLANT_TORQUE_DRIVEN = 0, 1
_llp = C.POINTER(C.c_longlong)
SENSOR_DOUBLES, SENSOR_STATE_DOUBLES, SENSOR_RECORD_DOUBLES = 16, 72, 8          # set_sensors: the setting, the state and the record of an instance
JOINT_DOUBLES, JOINT_STOP_DOUBLES, JOINT_RECORD_DOUBLES = 8, 2, 8                # set_joints: a joint, an instance's stops, its record
JOINT_RECORD_FIELDS = dict(substeps=0, substeps_beyond_range=1, max_excursion=2, max_friction_torque=3, max_motor_lag=4, joints_beyond_range=5)
WRENCH_EVENTS, WRENCH_DOUBLES, WRENCH_RECORD_DOUBLES = 8, 16, 8                  # set_wrenches: the most events per instance, an event, the record
WRENCH_RECORD_FIELDS = dict(substeps=0, substeps_active=1, events_acted=2, max_generalized_force=3, impulse=slice(4, 7))
FLAG_WRENCH = 16                    # bit 4 of the tick record's flags: a wrench event acted in a sub-step of the tick
COMMAND_EVENTS, COMMAND_DOUBLES, COMMAND_STATE_DOUBLES, COMMAND_RECORD_DOUBLES = 8, 28, 4, 32     # set_commands: events per instance, an event, state, record
COMMAND_RECORD_FIELDS = dict(updates=0, index=1, events_begun=2, latch_time=3, anchor=slice(4, 6), max_distance=6, sum_sq_distance=7, des=slice(8, 20))
SENSOR_RECORD_FIELDS = dict(ticks=0, samples=1, max_position=2, max_orientation=3, max_linear_velocity=4, max_angular_velocity=5, max_joint_angle=6,
                            max_joint_rate=7)


def _d(a):
    return a.ctypes.data_as(_dp)


def decode_ground_word(field63):
    """field 63 of a record (a number or an array of them) -> dict(ground=bool, in_contact, slipping, plan_differs), the last three with a trailing
    axis over the four feet.  ground is False (and the rest all False) for a record written without a ground, whose field 63 is 0"""
    w = np.asarray(field63).astype(np.int64)
    ground = w >= GROUND_WORD_OFFSET
    word = np.where(ground, w - GROUND_WORD_OFFSET, 0)
    bits = lambda first: ((word[..., None] >> (first + np.arange(4))) & 1).astype(bool)
    return dict(ground=ground, in_contact=bits(0), slipping=bits(4), plan_differs=bits(8))


def terrain_patch(x=(-np.inf, np.inf), y=(-np.inf, np.inf), z0=0.0, gx=0.0, gy=0.0, mu=0.6):
    """one patch of a terrain -> [8] = x_min, x_max, y_min, y_max, z0, gx, gy, mu: the rectangle x, y in world coordinates (unbounded by default),
    the surface z = z0 + gx x + gy y through the world origin, the friction coefficient.  x = (1, 0) makes an empty patch"""
    return np.array([x[0], x[1], y[0], y[1], z0, gx, gy, mu], float)


def publish_ticks(L, first_tick, ticks, ticks_per_update, tick_dt, base, per_iteration, iters):
    """the publication ticks of a rollout with a latency set, on the host (srbm_latency_publish_ticks_host; L: the loaded library, host.lib()).
    iters[batch][n_updates]: the IPM iterations of update u = 1 .. n_updates of every instance; base, per_iteration: one number or [batch].
    -> tick[batch][n_updates], overrun[batch][n_updates]: the tick before which update u is published and whether by force before it was due, for
    the publications among ticks first_tick .. first_tick + ticks - 1 of a rollout from tick 0; -1 and 0 for the others"""
    iters = np.ascontiguousarray(iters, dtype=np.int32)
    if iters.ndim != 2:
        raise ValueError('iters is [batch][n_updates]')
    batch, n = iters.shape
    lat = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(base, float), (batch,)), np.broadcast_to(np.asarray(per_iteration, float), (batch,))], axis=1))
    tick, over = np.zeros((batch, n), np.int32), np.zeros((batch, n), np.int32)
    if L.srbm_latency_publish_ticks_host(batch, int(first_tick), int(ticks), int(ticks_per_update), float(tick_dt), _d(lat),
                                         (iters if iters.size else np.zeros(1, np.int32)).ctypes.data_as(_ip), n, (tick if n else np.zeros(1, np.int32)).ctypes.data_as(_ip),
                                         (over if n else np.zeros(1, np.int32)).ctypes.data_as(_ip)) != 0:
        raise RuntimeError('srbm: ' + L.srbm_last_error().decode())
    return tick, over


class ControllerRollout:
    def __init__(self, mpc):
        self.mpc, self.L = mpc, mpc.L

    def reset(self, q_des):
        """MPCController's q_des_ for every instance, one q[19] or [batch][19] (srbm_control_tick_reset)"""
        m = self.mpc
        m._chk(self.L.srbm_control_tick_reset(m.h, _d(m._bcast(q_des, 19))))

    def set_state(self, q, v):
        """the plant's configuration q (one [19] or [batch][19]) and velocity v ([18] or [batch][18])"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_state(m.h, _d(m._bcast(q, 19)), _d(m._bcast(v, 18))))

    def state(self):
        """-> q[batch][19], v[batch][18] after the work queued so far"""
        m = self.mpc
        q, v = np.zeros((m.batch, 19)), np.zeros((m.batch, 18))
        m._chk(self.L.srbm_wb_plant_get_state(m.h, _d(q), _d(v)))
        return q, v

    def advance(self, first_tick, ticks, ticks_per_update, tick_dt, gait=None, gait_opt_freq=None):
        """ticks first_tick .. first_tick + ticks - 1 of period tick_dt: control tick, plant step, and after every tick k > 0 with
        k % ticks_per_update == 0 an MPC update at k * tick_dt that is in force from tick k + 1; asynchronous on the batch's stream.
        gait: a host.BatchGaitOptimizer of this batch -- update r = k / ticks_per_update is then a line search (r % gait_opt_freq == 0), an update
        followed by gradient and LP ((r + 1) % gait_opt_freq == 0) or a plain update (srbm_gait_controller_advance)"""
        if gait is None:
            if gait_opt_freq is not None:
                raise ValueError('gait_opt_freq without a gait optimiser')
            self.mpc._chk(self.L.srbm_controller_advance(self.mpc.h, int(first_tick), int(ticks), int(ticks_per_update), float(tick_dt)))
            return
        if gait.mpc is not self.mpc:
            raise ValueError('the gait optimiser belongs to another batch')
        if gait_opt_freq is None:
            raise ValueError('a gait optimiser without gait_opt_freq')
        self.mpc._chk(self.L.srbm_gait_controller_advance(gait.g, int(first_tick), int(ticks), int(ticks_per_update), float(tick_dt), int(gait_opt_freq)))

    # ---- contact feedback from the ground ----
    def set_contact_feedback(self, on):
        """MPC::AdjustForCurrentContacts on the ground's contact state before every MPC update of `advance` (which then requires the torque-driven
        plant with a ground); off by default"""
        self.mpc._chk(self.L.srbm_controller_set_contact_feedback(self.mpc.h, int(bool(on))))

    def contact_feedback(self):
        """-> fb[batch][4][2]: per foot the number of touch-downs moved since set_state and the time of the last move (-1: none)"""
        m = self.mpc
        fb = np.zeros((m.batch, 4, 2))
        m._chk(self.L.srbm_controller_get_contact_feedback(m.h, _d(fb)))
        return fb

    def contact_feedback_dev(self, time, cs):
        """the feedback kernel alone on device pointers (ints): time[batch], cs[batch][12]; asynchronous, counts in the feedback record"""
        self.mpc._chk(self.L.srbm_controller_contact_feedback_dev(self.mpc.h, time, cs))

    def plant_step_dev(self, tick, tick_dt, q, v, qp_sol, status):
        """the plant step alone on device pointers (ints): q[batch][19], v[batch][18] in place from qp_sol[batch][30], status[batch][2] of
        control_tick_dev; asynchronous, never logs"""
        self.mpc._chk(self.L.srbm_wb_plant_step_dev(self.mpc.h, int(tick), float(tick_dt), q, v, qp_sol, status))

    # ---- MPC computation latency ----
    def set_latency(self, base, per_iteration=0.0):
        """the latency between the start of an MPC update and the tick from which the control ticks see its result: base + per_iteration * (IPM
        iterations of the solve) seconds, each one number or [batch]; the ticks then read the published trajectories (srbm_controller_set_latency).
        base None removes the setting"""
        m = self.mpc
        if base is None:
            m._chk(self.L.srbm_controller_set_latency(m.h, None))
            return
        lat = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(base, float), (m.batch,)),
                                             np.broadcast_to(np.asarray(per_iteration, float), (m.batch,))], axis=1))
        m._chk(self.L.srbm_controller_set_latency(m.h, _d(lat)))

    def latency_record(self):
        """-> pub[batch][8] (LATENCY_RECORD_FIELDS) after the work queued so far"""
        m = self.mpc
        pub = np.zeros((m.batch, LATENCY_RECORD_DOUBLES))
        m._chk(self.L.srbm_controller_get_latency_record(m.h, _d(pub)))
        return pub

    def published(self, first=0, count=None):
        """the published trajectories, as BatchMPC.get_trajectory returns the MPC's"""
        m = self.mpc
        count = m.batch - first if count is None else count
        arr = (self.L.Trajectory * count)()          # host.Trajectory, hung on the loaded library by host.lib (this module does not import host.py)
        m._chk(self.L.srbm_controller_get_published(m.h, int(first), int(count), arr))
        return arr

    def publish_dev(self, time, update_number, t_start, force=0):
        """the publish kernel alone on a device pointer (int) time[batch]: update_number = (j - 1) // ticks_per_update of the tick j it precedes,
        t_start the start of that update, force 1 on a tick an update follows; asynchronous"""
        self.mpc._chk(self.L.srbm_controller_publish_dev(self.mpc.h, time, int(update_number), float(t_start), int(force)))

    # ---- sensor model ----
    def set_sensors(self, sens, seed=0):
        """the ticks read a measurement of the plant's (q, v) (srbm_controller_set_sensors): sens one [16] or [batch][16] (sensors.record builds one
        from physical values), seed one integer or [batch], 64 bits each.  sens None removes the setting"""
        m = self.mpc
        if sens is None:
            m._chk(self.L.srbm_controller_set_sensors(m.h, None, None))
            return
        sens = np.ascontiguousarray(np.broadcast_to(np.asarray(sens, float), (m.batch, SENSOR_DOUBLES)))
        seed = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64), (m.batch,))).view(np.int64)
        m._chk(self.L.srbm_controller_set_sensors(m.h, _d(sens), seed.ctypes.data_as(_llp)))

    def sensors(self):
        """-> sens[batch][16], seed[batch] (uint64) as set"""
        m = self.mpc
        sens, seed = np.zeros((m.batch, SENSOR_DOUBLES)), np.zeros(m.batch, np.int64)
        m._chk(self.L.srbm_controller_get_sensors(m.h, _d(sens), seed.ctypes.data_as(_llp)))
        return sens, seed.view(np.uint64)

    def sensor_state(self):
        """-> ms[batch][72]: the pose ring, the sample count and the filter memories (the table in include/srbm_rti.h) after the work queued so far"""
        m = self.mpc
        ms = np.zeros((m.batch, SENSOR_STATE_DOUBLES))
        m._chk(self.L.srbm_controller_get_sensor_state(m.h, _d(ms)))
        return ms

    def set_sensor_state(self, ms):
        m = self.mpc
        ms = np.ascontiguousarray(ms, float)
        if ms.shape != (m.batch, SENSOR_STATE_DOUBLES):
            raise ValueError('ms is [batch][%d]' % SENSOR_STATE_DOUBLES)
        m._chk(self.L.srbm_controller_set_sensor_state(m.h, _d(ms)))

    def sensor_record(self):
        """-> srec[batch][8] (SENSOR_RECORD_FIELDS) after the work queued so far"""
        m = self.mpc
        srec = np.zeros((m.batch, SENSOR_RECORD_DOUBLES))
        m._chk(self.L.srbm_controller_get_sensor_record(m.h, _d(srec)))
        return srec

    def measured(self):
        """-> qm[batch][19], vm[batch][18]: what the last tick read"""
        m = self.mpc
        q, v = np.zeros((m.batch, 19)), np.zeros((m.batch, 18))
        m._chk(self.L.srbm_controller_get_measured(m.h, _d(q), _d(v)))
        return q, v

    def measure_dev(self, tick, tick_dt, q, v, qm, vm):
        """the measure kernel alone on device pointers (ints): the true q[batch][19], v[batch][18] -> qm, vm; moves the batch's sensor state and record by
        tick `tick`; asynchronous"""
        self.mpc._chk(self.L.srbm_controller_measure_dev(self.mpc.h, int(tick), float(tick_dt), q, v, qm, vm))

    # ---- the torque-driven plant ----
    def set_plant(self, kind, kp=None, kd=None, torque_limit=None, substeps=1):
        """the plant `advance` launches: PLANT_QP_ACCELERATION (the default) or PLANT_TORQUE_DRIVEN.  kp, kd, torque_limit (one [12] or [batch][12])
        are the robot's actuator gains and limits, substeps the sub-steps per tick: set when one of the three is given (kp, kd None: 0;
        torque_limit None: no limit), else left as they are"""
        m = self.mpc
        if kp is not None or kd is not None or torque_limit is not None:
            lim = np.full(12, np.inf) if torque_limit is None else torque_limit
            m._chk(self.L.srbm_wb_plant_set_actuators(m.h, _d(m._bcast(np.zeros(12) if kp is None else kp, 12)),
                                                      _d(m._bcast(np.zeros(12) if kd is None else kd, 12)), _d(m._bcast(lim, 12)), int(substeps)))
        m._chk(self.L.srbm_wb_plant_set_kind(m.h, int(kind)))

    def set_plant_bodies(self, mass, com, inertia):
        """the plant's own bodies: mass [13] or [batch][13], com [13][3] or [batch][13][3], inertia [13][3][3] or [batch][13][3][3]"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_bodies_each(m.h, _d(m._bcast(mass, 13)), _d(m._bcast(com, 39)), _d(m._bcast(inertia, 117))))

    def forward_dynamics(self, q, v, tau, contact):
        """the constrained forward dynamics alone on the plant's bodies -> sol[batch][30] (a, then F stacked in foot order), status[batch]"""
        m = self.mpc
        con = np.ascontiguousarray(np.broadcast_to(np.asarray(contact, dtype=np.int32), (m.batch, 4)))
        sol, st = np.zeros((m.batch, 30)), np.zeros(m.batch, np.int32)
        m._chk(self.L.srbm_wb_forward_dynamics(m.h, _d(m._bcast(q, 19)), _d(m._bcast(v, 18)), _d(m._bcast(tau, 12)), con.ctypes.data_as(_ip), _d(sol),
                                               st.ctypes.data_as(_ip)))
        return sol, st

    def forward_dynamics_dev(self, q, v, tau, contact, sol, status):
        """the same on device pointers (ints); asynchronous"""
        self.mpc._chk(self.L.srbm_wb_forward_dynamics_dev(self.mpc.h, q, v, tau, contact, sol, status))

    def fd_step_dev(self, tick, tick_dt, q, v, control, contact, status, sol=None):
        """the torque-driven plant step alone on device pointers (ints): q[batch][19], v[batch][18] in place from control[batch][36],
        contact[batch][4], status[batch][2] of control_tick_dev; sol: None or [batch][30] <- (a, F) of the last sub-step; asynchronous, never logs"""
        self.mpc._chk(self.L.srbm_wb_fd_step_dev(self.mpc.h, int(tick), float(tick_dt), q, v, control, contact, status, sol))

    # ---- the joint model of the torque-driven plant ----
    def set_joints(self, joints, stops=None):
        """a joint model for the torque-driven plant (srbm_wb_plant_set_joints): joints one [12][8] or [batch][12][8], per joint b, I_a, f_c, v_s,
        q_min, q_max, T, 0 (joints.record builds one from physical values), stops one [2] or [batch][2] = k_l, d_l.  joints None removes the setting"""
        m = self.mpc
        if joints is None:
            m._chk(self.L.srbm_wb_plant_set_joints(m.h, None, None))
            return
        if stops is None:
            raise ValueError('a joint model needs the compliance of its stops: stops = (k_l, d_l)')
        m._chk(self.L.srbm_wb_plant_set_joints(m.h, _d(m._bcast(joints, 12 * JOINT_DOUBLES)), _d(m._bcast(stops, JOINT_STOP_DOUBLES))))

    def joints(self):
        """-> joints[batch][12][8], stops[batch][2] as set"""
        m = self.mpc
        j, s = np.zeros((m.batch, 12, JOINT_DOUBLES)), np.zeros((m.batch, JOINT_STOP_DOUBLES))
        m._chk(self.L.srbm_wb_plant_get_joints(m.h, _d(j), _d(s)))
        return j, s

    def joint_state(self):
        """-> js[batch][12]: the motor torques after the work queued so far"""
        m = self.mpc
        js = np.zeros((m.batch, 12))
        m._chk(self.L.srbm_wb_plant_get_joint_state(m.h, _d(js)))
        return js

    def set_joint_state(self, js):
        """one [12] or [batch][12] (set_joints and set_state reset it to zero)"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_joint_state(m.h, _d(m._bcast(js, 12))))

    def joint_record(self):
        """-> jrec[batch][8] (JOINT_RECORD_FIELDS) after the work queued so far"""
        m = self.mpc
        jrec = np.zeros((m.batch, JOINT_RECORD_DOUBLES))
        m._chk(self.L.srbm_wb_plant_get_joint_record(m.h, _d(jrec)))
        return jrec

    # ---- the wrench schedule of the torque-driven plant ----
    def set_wrenches(self, wrenches):
        """timed external wrenches on the bodies of the torque-driven plant (srbm_wb_plant_set_wrenches): wrenches[batch][n_events][16], or one
        [n_events][16] for every instance, 1 <= n_events <= 8 (wrenches.event and wrenches.schedule build them).  None removes the setting"""
        m = self.mpc
        if wrenches is None:
            m._chk(self.L.srbm_wb_plant_set_wrenches(m.h, None, 0))
            return
        w = np.asarray(wrenches, float)
        if w.ndim not in (2, 3) or w.shape[-1] != WRENCH_DOUBLES or (w.ndim == 3 and w.shape[0] != m.batch):
            raise ValueError('wrenches is [n_events][%d] or [batch][n_events][%d]' % (WRENCH_DOUBLES, WRENCH_DOUBLES))
        n = w.shape[-2]
        w = np.ascontiguousarray(np.broadcast_to(w, (m.batch, n, WRENCH_DOUBLES)))
        m._chk(self.L.srbm_wb_plant_set_wrenches(m.h, _d(w if w.size else np.zeros(1)), n))

    def wrenches(self):
        """-> wrenches[batch][n_events][16] as set"""
        m = self.mpc
        n = C.c_int(0)
        m._chk(self.L.srbm_wb_plant_get_wrenches(m.h, None, C.byref(n)))
        w = np.zeros((m.batch, n.value, WRENCH_DOUBLES))
        m._chk(self.L.srbm_wb_plant_get_wrenches(m.h, _d(w), C.byref(n)))
        return w

    def wrench_record(self):
        """-> wrec[batch][8] (WRENCH_RECORD_FIELDS) after the work queued so far"""
        m = self.mpc
        wrec = np.zeros((m.batch, WRENCH_RECORD_DOUBLES))
        m._chk(self.L.srbm_wb_plant_get_wrench_record(m.h, _d(wrec)))
        return wrec

    def wrench_force(self, time, q):
        """the generalized force of the events active at time (one number or [batch]: a sub-step time) on q ([19] or [batch][19])
        -> Q[batch][18], mask[batch] (bit e: event e is active)"""
        m = self.mpc
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(time, float), (m.batch,)))
        Q, mask = np.zeros((m.batch, 18)), np.zeros(m.batch, np.int32)
        m._chk(self.L.srbm_wb_wrench_force(m.h, _d(t), _d(m._bcast(q, 19)), _d(Q), mask.ctypes.data_as(_ip)))
        return Q, mask

    def wrench_force_dev(self, time, q, Q, mask):
        """the same on device pointers (ints): time[batch], q[batch][19] -> Q[batch][18], mask[batch] (int32); asynchronous"""
        self.mpc._chk(self.L.srbm_wb_wrench_force_dev(self.mpc.h, time, q, Q, mask))

    # ---- timed motion commands ----
    def set_commands(self, cmds):
        """the tracking target over time (srbm_controller_set_commands): cmds[batch][n_events][28], or one [n_events][28] for every instance,
        n_events <= 8 (srbm_loader.commands.hold / walk / stack build them).  None, or no events, removes the setting"""
        m = self.mpc
        if cmds is None:
            m._chk(self.L.srbm_controller_set_commands(m.h, None, 0))
            return
        c = np.asarray(cmds, float)
        if c.ndim not in (2, 3) or c.shape[-1] != COMMAND_DOUBLES or (c.ndim == 3 and c.shape[0] != m.batch):
            raise ValueError('cmds is [n_events][%d] or [batch][n_events][%d]' % (COMMAND_DOUBLES, COMMAND_DOUBLES))
        n = c.shape[-2]
        c = np.ascontiguousarray(np.broadcast_to(c, (m.batch, n, COMMAND_DOUBLES)))
        m._chk(self.L.srbm_controller_set_commands(m.h, _d(c if c.size else np.zeros(1)), n))

    def commands(self):
        """-> cmds[batch][n_events][28] as set ([batch][0][28]: none set)"""
        m = self.mpc
        n = C.c_int(0)
        m._chk(self.L.srbm_controller_get_commands(m.h, None, C.byref(n)))
        c = np.zeros((m.batch, n.value, COMMAND_DOUBLES))
        if n.value:
            m._chk(self.L.srbm_controller_get_commands(m.h, _d(c), C.byref(n)))
        return c

    def command_state(self):
        """-> cstate[batch][4] = latched event (-1: none), anchor x, anchor y, latch time, after the work queued so far"""
        m = self.mpc
        s = np.zeros((m.batch, COMMAND_STATE_DOUBLES))
        m._chk(self.L.srbm_controller_get_command_state(m.h, _d(s)))
        return s

    def set_command_state(self, cstate):
        m = self.mpc
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(cstate, float), (m.batch, COMMAND_STATE_DOUBLES)))
        m._chk(self.L.srbm_controller_set_command_state(m.h, _d(s)))

    def command_record(self):
        """-> crec[batch][32] (COMMAND_RECORD_FIELDS) after the work queued so far"""
        m = self.mpc
        r = np.zeros((m.batch, COMMAND_RECORD_DOUBLES))
        m._chk(self.L.srbm_controller_get_command_record(m.h, _d(r)))
        return r

    def command_costs(self):
        """-> w[batch][12], Phi_w[batch][12] of the records on the device after the work queued so far: what the last command wrote, or the host's"""
        m = self.mpc
        w, pw = np.zeros((m.batch, 12)), np.zeros((m.batch, 12))
        m._chk(self.L.srbm_controller_get_command_costs(m.h, _d(w), _d(pw)))
        return w, pw

    def command_dev(self, time, state):
        """the command kernel alone on device pointers (ints): time[batch], state[batch][13]; asynchronous.  Its place in a host-driven chain is
        before get_real_time_update_dev"""
        self.mpc._chk(self.L.srbm_controller_command_dev(self.mpc.h, time, state))

    # ---- the ground of the torque-driven plant ----
    def set_ground(self, ground):
        """a compliant ground under the torque-driven plant: one [8] or [batch][8] = z0 (-inf: none for the instance), k_n, d_n, mu, k_t, d_t, 0, 0;
        None removes it (kind 1 then holds the planned feet again)"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_ground(m.h, None if ground is None else _d(m._bcast(ground, GROUND_DOUBLES))))

    def set_terrain(self, terrain):
        """a terrain for the ground (set_ground first): [P][8] for every instance or [batch][P][8], 1 <= P <= TERRAIN_PATCHES, the rows as
        terrain_patch makes them; later patches lie over earlier ones.  None removes it (the ground is its plane again)"""
        m = self.mpc
        if terrain is None:
            m._chk(self.L.srbm_wb_plant_set_terrain(m.h, None, 0))
            return
        t = np.asarray(terrain, float)
        if t.ndim not in (2, 3) or t.shape[-1] != TERRAIN_DOUBLES or (t.ndim == 3 and t.shape[0] != m.batch):
            raise ValueError('a terrain is [patches][%d] or [batch][patches][%d]' % (TERRAIN_DOUBLES, TERRAIN_DOUBLES))
        t = np.ascontiguousarray(np.broadcast_to(t, (m.batch,) + t.shape[-2:]))
        m._chk(self.L.srbm_wb_plant_set_terrain(m.h, _d(t if t.size else np.zeros(1)), int(t.shape[1])))       # (no patches: refused there, not NULL)

    def contact_state(self):
        """-> cs[batch][4][3]: per foot in_contact (0 | 1; with a terrain 1 + the patch), anchor_x, anchor_y, after the work queued so far"""
        m = self.mpc
        cs = np.zeros((m.batch, 4, 3))
        m._chk(self.L.srbm_wb_plant_get_contact_state(m.h, _d(cs)))
        return cs

    def set_contact_state(self, cs):
        """one [4][3] or [batch][4][3] (set_state resets it to no foot in contact)"""
        m = self.mpc
        m._chk(self.L.srbm_wb_plant_set_contact_state(m.h, _d(m._bcast(cs, CONTACT_STATE_DOUBLES))))

    def ground_dynamics(self, q, v, tau, cs):
        """the contact law and the 18-row solve alone on the plant's bodies -> sol[batch][30] (a, then F[4][3] in foot order), cs_out[batch][4][3],
        status[batch]"""
        m = self.mpc
        sol, out, st = np.zeros((m.batch, 30)), np.zeros((m.batch, 4, 3)), np.zeros(m.batch, np.int32)
        m._chk(self.L.srbm_wb_ground_dynamics(m.h, _d(m._bcast(q, 19)), _d(m._bcast(v, 18)), _d(m._bcast(tau, 12)), _d(m._bcast(cs, CONTACT_STATE_DOUBLES)),
                                              _d(sol), _d(out), st.ctypes.data_as(_ip)))
        return sol, out, st

    def ground_dynamics_dev(self, q, v, tau, cs_in, sol, cs_out, status):
        """the same on device pointers (ints); asynchronous"""
        self.mpc._chk(self.L.srbm_wb_ground_dynamics_dev(self.mpc.h, q, v, tau, cs_in, sol, cs_out, status))

    def ground_step_dev(self, tick, tick_dt, q, v, cs, control, status, sol=None):
        """the ground step alone on device pointers (ints): q[batch][19], v[batch][18], cs[batch][12] in place from control[batch][36] and
        status[batch][2] of control_tick_dev; sol: None or [batch][30] <- (a, F) of the last sub-step; asynchronous, never logs"""
        self.mpc._chk(self.L.srbm_wb_ground_step_dev(self.mpc.h, int(tick), float(tick_dt), q, v, cs, control, status, sol))

    # ---- the tick log ----
    def tick_log_enable(self, max_ticks):
        """allocate max_ticks x batch records, cursor 0; 0 disables and frees"""
        self.mpc._chk(self.L.srbm_tick_log_enable(self.mpc.h, int(max_ticks)))

    def tick_log_reset(self):
        self.mpc._chk(self.L.srbm_tick_log_reset(self.mpc.h))

    def tick_log_count(self):
        n = C.c_int(0)
        self.mpc._chk(self.L.srbm_tick_log_count(self.mpc.h, C.byref(n)))
        return n.value

    def tick_log(self, first=0, count=None):
        """-> log[count][batch][TICK_LOG_DOUBLES] (synchronous)"""
        count = self.tick_log_count() - first if count is None else count
        a = np.zeros((count, self.mpc.batch, TICK_LOG_DOUBLES))
        self.mpc._chk(self.L.srbm_tick_log_get(self.mpc.h, int(first), int(count), _d(a)))
        return a

    def tick_log_copy_dev(self, ptr, first=0, count=None):
        """device to device on the batch's stream, no synchronisation"""
        count = self.tick_log_count() - first if count is None else count
        self.mpc._chk(self.L.srbm_tick_log_copy_dev(self.mpc.h, int(first), int(count), ptr))
