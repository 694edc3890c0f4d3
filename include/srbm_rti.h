/* C-ABI of the MI355X-native batched SRBM real-time-iteration path (libsrbm_rti.so).
 *
 * Every entry point replaces, for a BATCH of independent MPC instances, one public method of the reference's
 * mpc::MPC / mpc::MPCSingleRigidBody (cited per function, paths relative to /root/reference).  Instance b of the batch
 * is exactly one reference object: its constructor arguments (srbm_mpc_info + model constants: one set for every instance
 * through srbm_batch_create, one per instance through srbm_batch_create_each), its costs, the default contact schedule,
 * its state.  Plain pointers and sizes only; all array arguments are HOST pointers unless the function
 * name ends in _dev.  Return value: 0 on success, negative on error (srbm_last_error() gives the text).
 * The library fails loudly: there is no CPU fallback of any kind.
 */
#ifndef SRBM_RTI_H
#define SRBM_RTI_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct srbm_batch srbm_batch;

/* mpc::MPCInfo, mpc/include/mpc.h:39-62 (fields that affect the live SRBM path) */
typedef struct srbm_mpc_info {
    int num_nodes;
    double integrator_dt, friction_coef, force_bound, swing_height, foot_offset;
    double ee_box_size[2];
    double force_cost;
} srbm_mpc_info;

/* constants the reference reads from pinocchio at construction: mpc/models/model.cpp:27 (mass),
 * mpc/models/single_rigid_body_model.cpp:33-37 (Ir), :258-308 (hip joint origins, trunk frame, FL FR RL RR) */
typedef struct srbm_model {
    double mass;
    double Ir[9];
    double hip_xy[8];
} srbm_model;

/* MPCSingleRigidBody::MPCSingleRigidBody x batch  (mpc/mpc_single_rigid_body.cpp:9-23, mpc/mpc.cpp:38-76) */
int srbm_batch_create(srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, int device);
/* batch x MPCSingleRigidBody::MPCSingleRigidBody, each with its own constructor data: info[batch], model[batch].  Per instance: mass, Ir,
 * friction_coef, force_bound, force_cost, ee_box_size.  Batch-wide -- they fix the QP shapes, the time grid and the foot geometry --:
 * num_nodes, integrator_dt, swing_height, foot_offset and hip_xy; instances that disagree on one are refused with an error that names it
 * (checked before any device is probed).  The cost setters below then write every instance, their _each forms a range of instances. */
int srbm_batch_create_each(srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, int device);
/* read-back of instance inst's constructor data (force_cost: as last set by srbm_add_force_cost[_each]) */
int srbm_get_instance_model(const srbm_batch* h, int inst, srbm_mpc_info* info, srbm_model* model);
int srbm_batch_destroy(srbm_batch* h);
const char* srbm_last_error(void);

/* value semantics of the reference object: MPC::MPC(const MPC&) / operator= (mpc/mpc.cpp:1133-1181, mpc_single_rigid_body.cpp:
 * 804-807; the gait line search copies one MPC per thread, mpc/gait_optimizer.cpp:696).  The clone owns its own stream and
 * device buffers and carries the complete state of `src` (parameters, costs, tolerances, trajectories, last QP, plant). */
int srbm_batch_clone(const srbm_batch* src, srbm_batch** out);
int srbm_batch_size(const srbm_batch* h);
/* capacities of this build: cap4 = {max horizon nodes N, max spline variables n_u, max force samples, max knots per foot}.
 * libsrbm_rti.so: {50, 160, 120, 32}, the configurations the reference ships (its normal matrix lives in LDS);
 * libsrbm_rti_large.so (same sources, -DSRBM_LARGE): {100, 240, 200, 32}, the reference's own limit of 101 trajectory nodes
 * (mpc/include/trajectory.h:165-166); same C-ABI, same results, slower (normal matrix in L2). */
int srbm_get_capacity(int* cap4);
int srbm_num_nodes(const srbm_batch* h);

/* MPC::AddQuadraticTrackingCost (mpc/mpc.cpp:533-540): Q 12x12 row-major, state_des in tangent coordinates (12) */
int srbm_add_quadratic_tracking_cost(srbm_batch* h, const double* state_des12, const double* Q144);
/* MPC::SetQuadraticFinalCost / SetLinearFinalCost (mpc/mpc.cpp:137-151) */
int srbm_set_quadratic_final_cost(srbm_batch* h, const double* Phi144);
int srbm_set_linear_final_cost(srbm_batch* h, const double* w12);
/* MPC::AddForceCost (mpc/mpc.cpp:791-802): weight of every force spline variable (replaces srbm_mpc_info.force_cost) */
int srbm_add_force_cost(srbm_batch* h, double weight);
/* The four cost setters above write EVERY instance (the last write wins per instance).  Their _each forms are the same methods of the reference
 * objects [first, first + count) of the batch, one call per object folded into one: arrays [count][...] (state_des12 [count][12], Q144 and
 * Phi144 [count][144], w12 [count][12], weight [count]).  first / count out of range or a NULL array: error, the batch unchanged. */
int srbm_add_quadratic_tracking_cost_each(srbm_batch* h, int first, int count, const double* state_des12, const double* Q144);
int srbm_set_quadratic_final_cost_each(srbm_batch* h, int first, int count, const double* Phi144);
int srbm_set_linear_final_cost_each(srbm_batch* h, int first, int count, const double* w12);
int srbm_add_force_cost_each(srbm_batch* h, int first, int count, const double* weight);
/* MPC::SetStateTrajectoryWarmStart (mpc/mpc.cpp:700-706): states[batch][13], replicated over the horizon */
int srbm_set_state_trajectory_warm_start(srbm_batch* h, const double* states);
/* ClarabelInterface tolerances (mpc/qp/clarabel_interface.cpp:18-27,165-175) for the on-device IPM.
 * Defaults: the reference's own -- gap 1e-15, feasibility 1e-10 -- and 200 iterations (Clarabel's max_iter) */
int srbm_set_solver_tolerances(srbm_batch* h, double tol_gap_abs, double tol_gap_rel, double tol_feas, int max_iter);
/* Two OPT-IN settings of the on-device solver that have no counterpart in ClarabelInterface (mpc/qp/clarabel_interface.cpp:72-155 runs Clarabel
 * to its 1e-15 gap).  A new batch has both at 0: every solve then ends by exactly the gap criterion of srbm_set_solver_tolerances, i.e. the
 * reference's (clarabel_interface.cpp:165-175), its multipliers are at that tolerance and any solve may be differentiated afterwards.
 *   tol_step > 0: a solve ALSO ends Solved as soon as the affine Newton step -- which measures the distance of the iterate to the minimiser of
 *     the QP -- is below tol_step * max(1, |u|_inf); the iterate then takes that step (what is left is <= 0.2 tol_step).  Applies to EVERY
 *     launch path (srbm_get_real_time_update[_dev], srbm_rti_advance[_unfused], srbm_closed_loop_advance, the line-search candidates and the
 *     plain RTI steps of srbm_gait_rti_advance).  The primal point is then accurate to tol_step, the multipliers only to that order: a solve
 *     that ended through the rule is flagged (srbm_get_solve_flags bit 0), residuals / gap / QP cost reported for it are re-evaluated at the
 *     returned iterate, and srbm_gait_compute_sensitivity / _gradient REFUSE it (error return, not a silent valid = 0) -- srbm_gait_rti_advance
 *     runs the one solve it differentiates at the gap criterion by itself, a caller that drives that protocol passes tol_step = 0 first.
 *   start_mu > 0: every solve is first ATTEMPTED from the linearisation point (the shifted solution of the previous RTI step) with slacks
 *     h - G u and perfectly centred multipliers lambda = start_mu / s -- five to six decades further down the central path than Clarabel's
 *     starting point -- with an iteration budget, and repeated from the standard point unless the attempt ends Solved (through the step rule
 *     or, with tol_step = 0, through the gap criterion itself: (0, start_mu) keeps the reference's TERMINATION criterion for every solve and only
 *     changes where the iteration starts).  Honoured by the device-resident open-loop launch srbm_rti_advance ONLY (there a repeated attempt of
 *     one instance is averaged over its K steps and the state is node 1 of the plan); IGNORED by srbm_get_real_time_update[_dev],
 *     srbm_rti_advance_unfused, srbm_create_initial_run (one-step launches wait for the slowest instance every time), by
 *     srbm_closed_loop_advance (integration error and pushes make the attempts fail) and by srbm_gait_rti_advance (its candidates belong to
 *     other contact schedules).
 * bench.py's headline runs (0, SRBM_FAST_START_MU): the reference's termination criterion, every solve of srbm_rti_advance first attempted from
 * the linearisation point.  Its named secondary object runs (SRBM_FAST_TOL_STEP, SRBM_FAST_START_MU) (1e-4 relative primal accuracy is the bar
 * of the path), and the same line carries the run at (0, 0).  Parity of every mode: tests/test_gpu_resync.py, DESIGN.md sections 3-4. */
#define SRBM_FAST_TOL_STEP 1e-5
#define SRBM_FAST_START_MU 0.1
int srbm_set_solver_step_rule(srbm_batch* h, double tol_step, double start_mu);
int srbm_get_solver_step_rule(const srbm_batch* h, double* tol_step, double* start_mu);
/* flags[batch] of the LAST solve: bit 0 = ended through the step rule (duals not at the gap tolerance), bit 1 = began with a lower-start attempt,
 * bit 2 = that attempt was repeated from the standard starting point */
int srbm_get_solve_flags(srbm_batch* h, int* flags);

/* MPC::CreateInitialRun (mpc/mpc.cpp:78-90): 10 solves at t = 0.   state[batch][13], ee[batch][4][3] */
int srbm_create_initial_run(srbm_batch* h, const double* state, const double* ee_start_locations);
/* MPC::GetRealTimeUpdate (mpc/mpc.cpp:92-108) == one MPCSingleRigidBody::Solve (mpc_single_rigid_body.cpp:25-216).
 * init_time[batch] */
int srbm_get_real_time_update(srbm_batch* h, const double* state, const double* init_time, const double* ee_start_locations);
/* same, inputs already resident in HBM (device pointers), asynchronous on the handle's stream */
int srbm_get_real_time_update_dev(srbm_batch* h, const double* state_dev, const double* init_time_dev, const double* ee_dev);
/* Device-resident open-loop protocol of test/gait_opt_playground.cpp:113-126: `steps` RTI iterations with
 * state := node 1 of the previous trajectory, foot locations := previous trajectory at t, t_i = (first_index+i)*dt.
 * No host round trip between iterations.  Asynchronous; srbm_synchronize() to wait.
 * The open-loop entries (this one, srbm_rti_advance_unfused, srbm_gait_rti_advance) ignore srbm_plant_set_period: "state := node 1 of the previous
 * trajectory" has no meaning at another period than the node step.
 * A batch of at most one instance per CU runs as one workgroup per instance for all steps; a LARGER batch with steps > 1 runs on a resident grid
 * that takes (instance, step) items from per-XCD queues (csrc/srbm_fused.hiph: the launch no longer ends with the instance whose `steps` solves
 * happen to be the longest) -- bitwise the same results (tests/test_gpu_queue.py), and bitwise those of the same steps launched one at a time
 * (tests/test_gpu_launch_equivalence.py); launches of more than 32 767 steps and SRBM_NO_STEP_QUEUE=1 in the environment at srbm_create time
 * select the first form.  The same holds for srbm_closed_loop_advance. */
int srbm_rti_advance(srbm_batch* h, int first_index, int steps);
/* same protocol with one kernel launch per phase and step (A/B measurements against the fused kernel) */
int srbm_rti_advance_unfused(srbm_batch* h, int first_index, int steps);

/* ---- closed-loop rollout harness ----
 * What the reference closes over MuJoCo (test/simulation_mpc.cpp:186-215), device resident for a batch: the plant is
 * the single-rigid-body model itself, SingleRigidBodyModel::CalcDynamics (mpc/models/single_rigid_body_model.cpp:
 * 222-256) integrated by RKIntegrator::CalcIntegral (mpc/rk_integrator.cpp:14-30: explicit Euler on the tangent state)
 * under the forces and foot locations of the current trajectory, plus one push (momentum impulse) per instance.
 * Iteration i, t = (first_index+i)*dt (the current trajectory must start at t, e.g. first_index = 0 after
 * srbm_create_initial_run at time 0):
 *     x <- CalcIntegral(x, trajectory, t, substeps steps of dt/substeps)     advance_time = 0: every sub-step at time t
 *                                                                            (as coded), 1: time moves with the sub-steps
 *     if t < push_time <= t+dt:  lin-mom += impulse[0..2], ang-mom += impulse[3..5]
 *     MPC::GetRealTimeUpdate(x, t+dt, foot locations of the trajectory at t+dt)
 * srbm_plant_set_state: x[batch][13] (manifold state, as srbm_create_initial_run); srbm_plant_set_push: time[batch],
 * impulse[batch][6], both NULL to clear.  srbm_closed_loop_advance is asynchronous like srbm_rti_advance.
 *
 * The MPC period.  The reference's controller starts an update whenever the state sample is newer than the last one
 * (MPCController::MPCUpdate, controllers/mpc_controller.cpp:299-346; the comparison against integrator_dt is commented out on line 308): the solve
 * runs at the solve rate, the window shifts by a fraction of a node, the knots enter and leave it at arbitrary phases.  srbm_plant_set_period
 * gives every instance its own period p = period[b]; srbm_closed_loop_advance, srbm_plant_advance and srbm_gait_closed_loop_advance then run
 * iteration i (the gait entry: i = r - 1 of run r) of instance b as
 *     time  = i * p
 *     x    <- CalcIntegral(x, trajectory, time, substeps steps of p / substeps)
 *     push if time < push_time <= time + p
 *     solve at init_time = time + p, foot locations of the trajectory at time + p
 * and gait_opt_freq keeps counting runs, as the reference's run_num does.  Without a call, after NULL, or with every entry equal to dt, all
 * results are bitwise the same: the node step is the period where none is set.  Refused before anything is copied, the batch untouched and
 * the message naming the instance: a period that is not finite, <= 0, or >= num_nodes * dt (the plant would read past the trajectory).
 * srbm_batch_clone carries the setting.  The open-loop entries ignore it (see srbm_rti_advance). */
int srbm_plant_set_state(srbm_batch* h, const double* state);
int srbm_plant_get_state(srbm_batch* h, double* state);
int srbm_plant_set_push(srbm_batch* h, const double* time, const double* impulse);
/* MPC period of the closed-loop protocols, per instance: period[batch] seconds, NULL to clear (= the node step dt). */
int srbm_plant_set_period(srbm_batch* h, const double* period);
int srbm_plant_get_period(srbm_batch* h, double* period);   /* dt where none is set */
int srbm_closed_loop_advance(srbm_batch* h, int first_index, int steps, int substeps, int advance_time);
/* The plant half of iteration `index` on its own: integrate from index*p to index*p + p (p: the instance's MPC period, dt unless set), apply the push, fill the device input buffers of the
 * next solve -- and run NO solve.  Bitwise the inputs srbm_closed_loop_advance(h, index, 1, ..) hands to its solve, so a host may drive the loop
 * itself: srbm_plant_advance, then any entry that takes (state, init_time, ee).  Synchronous; outputs state[batch][13], time[batch] (= the
 * init_time of the next solve), ee[batch][4][3], any of them may be NULL.  Never logs. */
int srbm_plant_advance(srbm_batch* h, int index, int substeps, int advance_time, double* state, double* time, double* ee);
int srbm_synchronize(srbm_batch* h);
void* srbm_stream(srbm_batch* h);            /* hipStream_t the kernels are launched on */

/* ---- the step log: every step of a multi-step launch, kept on the device ----
 * A K-step launch leaves only its LAST solve in the read-back entries (status, stats, QP cost, merit, solve flags, plant state, the trajectory).
 * With a log enabled, every solve of srbm_rti_advance, srbm_closed_loop_advance (both launch forms), srbm_rti_advance_unfused and
 * srbm_get_real_time_update[_dev] also writes one record per instance, with no host round trip: the multi-step kernels write it after the update
 * phase of each step, the one-step entries through one small kernel behind their four.  srbm_gait_closed_loop_advance writes one record per run
 * and instance (fields 58..63 are its own, see there).  srbm_create_initial_run, srbm_plant_advance, every other srbm_gait_* entry
 * (srbm_gait_rti_advance included) and the line-search candidates never log.  Logging changes no result (tests/test_gpu_step_log.py,
 * tests/test_gpu_gait_closed_loop.py: bitwise).
 * The log is log[slot][batch][SRBM_STEP_LOG_DOUBLES]; a call of `steps` steps fills the slots [cursor, cursor + steps) and moves the cursor.  One
 * record, integers stored as doubles:
 *     index     content                                                                   the one-step read-back it equals
 *     0         the instance's solve count after this solve (the 'Solve #' column)
 *     1         init_time handed to the solve
 *     2, 3, 4   status, error bits of this solve, solve flags                             srbm_get_status, srbm_get_solve_flags
 *     5, 6      n, m                                                                      srbm_get_sizes columns 0, 1
 *     7..14     alpha, cost, dynamics defect, step norm, IPM iterations,                  srbm_get_stats, in its order
 *               primal residual, dual residual, gap
 *     15, 16    QP cost, merit dd                                                         srbm_get_qp_cost, srbm_get_merit (merit_dd)
 *     17..29    the state handed to the solve [13]: under a plant its state after         srbm_plant_get_state
 *               integration and push, open loop node 1 of the previous trajectory
 *     30..41    the foot locations handed to the solve [4][3]
 *     42..53    Trajectory::GetForce(ee, init_time) of the NEW trajectory [4][3]          srbm_eval_trajectory at init_time
 *     54..57    the contact flags of the new trajectory at init_time [4]                  srbm_eval_trajectory at init_time
 *     58..63    0 from every entry but srbm_gait_closed_loop_advance, which writes:
 *     58        kind of the run for this instance: 0 plain, 1 gradient and LP, 2 line search
 *               with a ready gradient (an instance that was not ready at a line-search run
 *               took the plain update and gets 0)
 *     59        the ready flag after the run
 *     60, 61    lp_status, pred_red (kind 1 only, else 0)                                 srbm_gait_get_lp_result
 *     62, 63    imin, the winner's cost / n (kind 2 only, else 0)                         srbm_gait_get_line_search_result
 * The merit is not a field: it is cost + 5000 * defect (fields 8 and 9) formed on the host, as srbm_get_merit forms it.  The evaluation behind
 * 42..57 reads the instance only (its error bits stay as the solve left them); a foot whose spline lookup fails gets NaN forces and flag -1.
 * srbm_step_log_enable allocates max_steps x batch records and sets the cursor to 0; max_steps = 0 disables logging and frees the buffer.  A call
 * whose steps do not fit the remaining capacity fails before anything is launched (srbm_last_error says how much room there is) and leaves the
 * batch untouched.  srbm_step_log_get (host, synchronous: out[count][batch][64]) and srbm_step_log_copy_dev (device to device on the batch's
 * stream, no synchronisation) fail for a slot range outside [0, steps_logged) and when no log is enabled.  A clone has logging off.
 * srbm_debug_get_launch_info reports a logged launch by the code of its unlogged twin. */
#define SRBM_STEP_LOG_DOUBLES 64
int srbm_step_log_record_doubles(void);                          /* SRBM_STEP_LOG_DOUBLES; callable without a GPU */
int srbm_step_log_enable(srbm_batch* h, int max_steps);
int srbm_step_log_reset(srbm_batch* h);                          /* cursor 0, buffer kept */
int srbm_step_log_count(srbm_batch* h, int* steps_logged);
int srbm_step_log_get(srbm_batch* h, int first_slot, int count, double* out);
int srbm_step_log_copy_dev(srbm_batch* h, int first_slot, int count, double* out_dev);

/* ---- rollout summaries: the step log folded into one outcome record per instance, on the device ----
 * What a disturbance-rejection study asks of a rollout -- did the instance fall, from when on was it back inside a band round its target, how far did it
 * get, how close to the friction pyramid did the forces come, how many solves failed -- without copying the log to the host.  The fold is INCREMENTAL:
 * log a chunk of steps, srbm_rollout_summary_fold, srbm_step_log_reset, repeat; a rollout of any length then needs a log of one chunk, and the
 * summaries are bit for bit independent of the chunking (every sum is accumulated in slot order).  The entries only read the log: no result changes.
 *
 * criteria[8], one set for the batch (a record's state is log fields 17..29: position p 17..19, linear momentum h 20..22, quaternion xyzw 23..26,
 * angular momentum L 27..29; ref[batch][6] = {p_ref[3], h_ref[3]} per instance).  Deviations are squared and the tilt is measured as
 * u = 2 (qx qx + qy qy) = 1 - cos(tilt): the fold uses no division, square root or transcendental.
 *     0  z_min        fallen if p_z < z_min
 *     1  tilt_max     fallen if u > tilt_max
 *     2  r2_settle    in band needs d2 = dx dx + dy dy <= r2_settle, dx = p_x - ref_x, dy likewise
 *     3  dz_settle    in band needs |p_z - ref_z| <= dz_settle
 *     4  tilt_settle  in band needs u <= tilt_settle
 *     5  h2_settle    in band needs |h - h_ref|^2 <= h2_settle
 *     6, 7            reserved, must be 0
 * A record is in band when all four conditions hold.  A comparison with a NaN is false: a NaN never becomes a maximum or a minimum.
 *
 * One summary, SRBM_ROLLOUT_SUMMARY_DOUBLES doubles, integers stored as doubles.  k is the 0-based ordinal of a record among those folded since the
 * last reset.  After a reset: counts and sums 0, every maximum -inf, every minimum +inf, every ordinal -1.  Where two records tie, the first keeps the
 * ordinal.  mu is the instance's own friction coefficient.
 *     0         records folded
 *     1, 2      solve number (log field 0) of the first and of the last record
 *     3, 4      init_time of the first and of the last record
 *     5, 6      count of status != Solved; ordinal of the first such record
 *     7         count of status > SolvedInacc
 *     8         bitwise OR of the error bits (a field that holds no set of bits -- negative, 2^53 or more, NaN -- adds nothing)
 *     9, 10     sum and max of the IPM iterations
 *     11        sum of the cost (log field 8)
 *     12        max dynamics defect
 *     13        min alpha
 *     14        max step norm
 *     15, 16    min and max of p_z
 *     17, 18    max d2 and the ordinal of its first occurrence
 *     19, 20    max u and its ordinal
 *     21        max |h - h_ref|^2
 *     22        max |L|^2
 *     23        ordinal of the first fallen record
 *     24        ordinal of the last record NOT in band
 *     25        count of in-band records
 *     26        max f_z over the feet (log fields 44, 47, 50, 53)
 *     27        min over records and feet with contact flag 1 of mu f_z - max(|f_x|, |f_y|)
 *     28        count of records with a NaN among log fields 17..29 and 42..57: such a record is counted here and in 0..14 (and 38..42), and takes no
 *               part in 15..37
 *     29        count of records whose four contact flags differ from those of the record folded before it (among the records that take part)
 *     30..33    the flags folded last: the carry; the first record sets it and counts no switch
 *     34..37    per foot, count of records with flag 1
 *     38, 39    count of gait runs of kind 1 and of kind 2 (log field 58)
 *     40        sum of pred_red over the kind-1 records
 *     41        count of kind-2 records with imin > 0
 *     42        the winner's cost / n of the last kind-2 record
 *     43..63    0
 * Derived, stated here once: "settled from" = field 24 + 1; an instance is SETTLED if field 23 < 0 and field 24 < field 0 - 1 (it did not fall and its
 * last record is in band); it has FALLEN if field 23 >= 0.
 *
 * One study record, SRBM_ROLLOUT_STUDY_DOUBLES doubles, of summaries[instances][64] taken in ascending instance order:
 *     0         instances
 *     1, 2      number fallen, number settled
 *     3         number with summary field 7 > 0
 *     4, 5      max (-1 where none is settled) and sum of "settled from" over the settled instances
 *     6, 7      max of summary field 17, of summary field 19
 *     8         min of summary field 27
 *     9         sum of summary field 9
 *     10        OR of summary field 8
 *     11..15    0
 *
 * srbm_rollout_summary_enable: criteria[8] and ref[batch][6]; allocates the summaries and resets them; criteria == NULL disables them and frees the
 * buffers.  srbm_rollout_summary_fold folds the log slots [first_slot, first_slot + count), which must lie in [0, steps_logged), asynchronously on the
 * batch's stream like the advance entries: a logged launch, a fold and srbm_step_log_reset need no host synchronisation between them, the writes of the
 * next launch are ordered behind the fold.  srbm_rollout_summary_get (synchronous): out[count][64] of instances [first, first + count);
 * srbm_rollout_summary_copy_dev: all of them device to device on the stream, no synchronisation.  srbm_rollout_study (synchronous) reduces the batch's own
 * summaries, srbm_rollout_study_dev (asynchronous) any device array of them -- the result of srbm_rollout_allgather_dev, which is srbm_allgather_results
 * for summaries: in place, rank r's batch x 64 doubles to rows [r * batch, (r + 1) * batch) of out_dev[world * batch][64], one ncclAllGather.
 * srbm_rollout_fold_host and srbm_rollout_study_host run the same fold of one record and the same reduction compiled for the host, on host arrays:
 * log[slots][batch][64], mu[batch], summaries[batch][64] in and out (the caller sets them to the reset state above); no GPU, no batch.
 * Refused before anything is queued, the batch and the summaries untouched, srbm_last_error naming the case: no step log enabled; no summary enabled; a
 * slot or instance range outside what exists; NULL where it is not allowed; a criterion that is not finite; a reserved criterion other than 0.
 * A clone has summaries off, as it has logging off. */
#define SRBM_ROLLOUT_SUMMARY_DOUBLES 64
#define SRBM_ROLLOUT_CRITERIA_DOUBLES 8
#define SRBM_ROLLOUT_REF_DOUBLES 6
#define SRBM_ROLLOUT_STUDY_DOUBLES 16
int srbm_rollout_summary_doubles(void);                        /* SRBM_ROLLOUT_SUMMARY_DOUBLES; callable without a GPU */
int srbm_rollout_summary_enable(srbm_batch* h, const double* criteria, const double* ref);
int srbm_rollout_summary_reset(srbm_batch* h);
int srbm_rollout_summary_fold(srbm_batch* h, int first_slot, int count);
int srbm_rollout_summary_get(srbm_batch* h, int first, int count, double* out);
int srbm_rollout_summary_copy_dev(srbm_batch* h, double* out_dev);
int srbm_rollout_study(srbm_batch* h, double* study);
int srbm_rollout_study_dev(srbm_batch* h, const double* summaries_dev, int instances, double* study_dev);
int srbm_rollout_fold_host(const double* log, int slots, int batch, int first_slot, int count, const double* criteria, const double* ref, const double* mu, double* summaries);
int srbm_rollout_study_host(const double* summaries, int instances, double* study);

/* ---- mpc::Trajectory as a flat record (mpc/include/trajectory.h:20-175): what MPC::GetTrajectory returns by value and
 * MPC::SetWarmStartTrajectory takes.  Knot tables as srbm_get_knots: kind 0 lift-off, 1 touch-down, 2 stance-interior
 * (force node with value + slope/FORCE_MULT), 3 mid-swing; force[ee][coord][knot] = {value, slope/100} (used on kind-2
 * knots), pos_xy[ee][coord][knot] (used on kind-0/1 knots); z follows from swing_height / foot_offset
 * (trajectory.cpp:303-317). */
#define SRBM_TRAJ_KMAX 32
#define SRBM_TRAJ_NODES_MAX 101          /* trajectory.h:165-166 */
typedef struct srbm_trajectory {
    int num_states;                       /* num_nodes + 1 */
    int nk[4];
    int knot_kind[4][SRBM_TRAJ_KMAX];
    double init_time, node_dt, swing_height, foot_offset;
    double states[SRBM_TRAJ_NODES_MAX][13];
    double knot_time[4][SRBM_TRAJ_KMAX];
    double force[4][3][SRBM_TRAJ_KMAX][2];
    double pos_xy[4][2][SRBM_TRAJ_KMAX];
} srbm_trajectory;
/* sizeof(srbm_trajectory) as the library was compiled: bindings check their own struct layout against it */
int srbm_sizeof_trajectory(void);
/* MPC::GetTrajectory (mpc/mpc.cpp:1023-1025) for instances [first, first + count): out[count] */
int srbm_get_trajectory(srbm_batch* h, int first, int count, srbm_trajectory* out);
/* MPC::SetWarmStartTrajectory (mpc/mpc.cpp:110-119) for instances [first, first + count): prev_traj_ = trajectory,
 * init_time_ = trajectory.GetTime(0).  The record is validated (knot counts, kinds, ordering); -1 on a malformed one.  The solver's memory of the instance (the back-off
 * of the lower-start attempts, srbm_set_solver_step_rule) is reset: two instances given the same trajectory solve the same next QP bit for bit. */
int srbm_set_warm_start_trajectory(srbm_batch* h, int first, int count, const srbm_trajectory* trajs);
/* Trajectory::GetForce / GetEndEffectorLocation / GetContacts at a time (mpc/trajectory.cpp:395-410, :70-80): pure host
 * arithmetic on a record (no GPU needed) -- what controllers/mpc_controller.cpp:171-186,352,415-509 evaluates at 1 kHz.
 * force[3], pos[3]; returns 0, or the error bits of the lookup (time outside the knot range: the reference throws). */
int srbm_trajectory_eval(const srbm_trajectory* traj, int ee, double time, double* force3, double* pos3, int* in_contact);
/* Trajectory::SplinesAsVec (mpc/trajectory.cpp:429-452) of a record: force spline variables (per foot, per coordinate: value and slope / FORCE_MULT of
 * every stance-interior knot) then position variables (per foot, x then y: the mutable nodes) -- the order of the spline part of the QP's decision
 * vector.  out[capacity]; *n_total = entries written, *n_force (may be NULL) = how many of them are force variables.  Host arithmetic. */
int srbm_trajectory_splines_as_vec(const srbm_trajectory* t, double* out, int capacity, int* n_total, int* n_force);
/* SingleRigidBodyModel::ConvertManifoldStateToTangentState / ConvertTangentStateToManifoldState (mpc/models/single_rigid_body_model.cpp:188-220;
 * used by the caller at controllers/mpc_controller.cpp:60): [p, lin-mom, quat xyzw, ang-mom] (13) <-> [p, lin-mom, log3(quat), ang-mom] (12).
 * Host arithmetic, the same functions the kernels use; the reference's ref_state argument is unused there (its quat_ref is the identity). */
int srbm_convert_manifold_to_tangent(const double* state13, double* tangent12);
int srbm_convert_tangent_to_manifold(const double* tangent12, double* state13);
/* the same for the CURRENT trajectory of every instance on the device: time[batch] -> force[batch][4][3], pos[batch][4][3],
 * in_contact[batch][4] (any output may be NULL) */
int srbm_eval_trajectory(srbm_batch* h, const double* time, double* force, double* pos, int* in_contact);
/* ... the same on DEVICE pointers (one launch on the batch's stream, no copy, no synchronisation): the contact flags the whole-body QP of the
 * same tick takes (srbm_qp_control_dev) without a round trip through the host; all four pointers required */
int srbm_eval_trajectory_dev(srbm_batch* h, const double* time_dev, double* force_dev, double* pos_dev, int* in_contact_dev);
/* MPCSingleRigidBody::GetEEBoxCenter (mpc/mpc_single_rigid_body.cpp:502-509): centers[4][2] = GetCOMToHip(ee).xy */
int srbm_get_ee_box_center(const srbm_batch* h, double* centers);
/* MPC::GetCost (cost of prev_qp_sol, cost[batch]) and MPC::GetAvgCost (mpc/mpc.cpp:991-998: mean over all solves so far) */
int srbm_get_cost(srbm_batch* h, double* cost);
int srbm_get_avg_cost(srbm_batch* h, double* avg_cost);
/* MPC::GetMeritValue / GetMeritGradient of the last solve (mpc/mpc.cpp:749-753, :783-788): the 'Merit' and 'Merit dd' columns of
 * MPC::PrintStatLineToFile; merit_dd may be NULL */
int srbm_get_merit(srbm_batch* h, double* merit, double* merit_dd);

/* MPC::UpdateContactTimes (mpc/mpc.cpp:1085-1088): times[batch][4][max_contacts], counts must match the current
 * number of contact knots of every foot */
int srbm_update_contact_times(srbm_batch* h, const double* times, int max_contacts);

/* MPC::AdjustForCurrentContacts (mpc/mpc.cpp:1195-1203) -> EndEffectorSplines::SetToTouchdown
 * (mpc/spline/end_effector_splines.cpp:1042-1060): time[batch], in_contact[batch][4] (0/1 per foot) */
int srbm_adjust_for_current_contacts(srbm_batch* h, const double* time, const int* in_contact);

/* ---- bilevel (gait) step: mpc::GaitOptimizer (mpc/include/gait_optimizer.h:20-170) for every instance of a batch ----
 * Contact-time vectors are laid out as in the reference's QP vector (gait_optimizer.cpp:395-408): foot after foot,
 * counts[batch][4] contact times per foot, row stride SRBM_GAIT_NV = 32 doubles per instance. */
#define SRBM_GAIT_NV 32
#define SRBM_GAIT_LS_SIZE 10      /* gait_optimizer.h:164 */
typedef struct srbm_gait srbm_gait;
/* GaitOptimizer::GaitOptimizer + UpdateSizes (gait_optimizer.cpp:15-63): allocates the 10 line-search candidates per instance */
int srbm_gait_create(srbm_batch* h, srbm_gait** out);
int srbm_gait_destroy(srbm_gait* g);
/* GaitOptimizer::SetContactTimes(mpc.GetTrajectory().GetContactTimes()) (gait_optimizer.cpp:395-408, mpc_controller.cpp:528) */
int srbm_gait_set_contact_times_from_trajectory(srbm_gait* g);
int srbm_gait_get_contact_times(srbm_gait* g, double* xk, int* counts);
/* MPC::ComputeDerivativeTerms -> ClarabelInterface::Computedx (mpc/mpc.cpp:1047-1069, mpc/qp/clarabel_interface.cpp:262-612):
 * KKT sensitivity of the last QP solution, d[batch][ld] = [dz (n); dlam (n_ineq, constraint order); dnu (n_eq)] */
int srbm_gait_compute_sensitivity(srbm_gait* g);
int srbm_gait_get_sensitivity(srbm_gait* g, double* d, int ld);
/* The gradient of the optimal cost w.r.t. the contact times (mpc_controller.cpp:518-561): SetContactTimes,
 * ComputeDerivativeTerms, MPCSingleRigidBody::ComputeParamPartialsClarabel for every contact time (mpc_single_rigid_body.cpp:
 * 642-792) and GaitOptimizer::ComputeCostFcnDerivWrtContactTimes (gait_optimizer.cpp:92-179).  dHdth[batch][32];
 * valid[batch] = 0 where the reference refuses (last QP not Solved, mpc.cpp:1048) -- may be NULL */
int srbm_gait_compute_gradient(srbm_gait* g);
int srbm_gait_get_gradient(srbm_gait* g, double* dHdth, int* valid);
/* a gradient supplied by the caller (the twin of srbm_gait_set_step): dHdth[batch][32], valid[batch]; what srbm_gait_optimize_contact_times
 * then minimises and srbm_gait_rti_advance's deriv_ready reads */
int srbm_gait_set_gradient(srbm_gait* g, const double* dHdth, const int* valid);
/* MPCSingleRigidBody::ComputeParamPartialsClarabel (mpc/mpc_single_rigid_body.cpp:642-792; read as matrices at test/mpc_test.cpp:181-184 and
 * mpc/gait_optimizer.cpp:92-179): partials of the QP of the last solve of instance `inst` w.r.t. contact time `idx` of foot `ee`, on the instance's
 * current trajectory, dense, in the layout of mpc::QPPartials (mpc/include/qp/qp_partials.h:15-35): dA [n_eq][n], dG [n_ineq][n], db [n_eq],
 * dh [n_ineq] (zero as coded); sizes from srbm_get_sizes.  Debug path like srbm_export_qp (the gradient kernel contracts the same entries on the fly). */
int srbm_gait_get_param_partials(srbm_batch* h, int inst, int ee, int idx, double* dA, double* dG, double* db, double* dh);
/* GaitOptimizer::OptimizeContactTimes (gait_optimizer.cpp:185-364): the LP  min dHdth' s  over the polytope of
 * gait_optimizer.cpp:410-534 at time[batch]; the step stays on the device for the line search.
 * lp_status[batch]: 0 solved, 1 iteration limit, 2 numerical failure (the reference throws "Bad gait optimization
 * solve"); pred_red[batch] = -dHdth' s (gait_optimizer.cpp:352-356) */
int srbm_gait_optimize_contact_times(srbm_gait* g, const double* time);
int srbm_gait_get_lp_result(srbm_gait* g, int* lp_status, double* pred_red);
/* step of the outer problem (result of OptimizeContactTimes, or supplied by the caller): step[batch][32] */
int srbm_gait_set_step(srbm_gait* g, const double* step);
int srbm_gait_get_step(srbm_gait* g, double* step);
/* GaitOptimizer::LineSearch (gait_optimizer.cpp:671-753): 10 schedules x_k + (i/10) step per instance, each a full
 * MPC::GetRealTimeUpdate(state, time, ee) on a copy of the instance (inputs as srbm_get_real_time_update); the cheapest
 * candidate (cost / n, primal-infeasible ones excluded, index 0 if all are) is installed with
 * MPC::SetWarmStartTrajectory.  imin[batch], costs[batch][10] may be NULL.
 * Refused, with nothing launched, on a handle that has not read contact times since srbm_gait_create (x_k would be the zeros of the
 * allocation): srbm_gait_set_contact_times_from_trajectory reads them, and so do srbm_gait_compute_gradient and the gradient runs of
 * srbm_gait_rti_advance, srbm_gait_closed_loop_advance and srbm_gait_controller_advance.  (The line-search runs of those three entries need no
 * contact times in the handle for an instance that is not ready: its candidates keep the instance's schedule bit for bit.) */
int srbm_gait_line_search(srbm_gait* g, const double* state, const double* init_time, const double* ee, int* imin, double* costs);
/* The MPC loop of the controller with the gait step folded in (controllers/mpc_controller.cpp:320-346), device
 * resident and open loop like srbm_rti_advance (test/gait_opt_playground.cpp:113-126): for run_num = first_run_num ...
 *   run_num % gait_opt_freq == 0, run_num > 0 : GaitOptimizer::LineSearch where a gradient is ready (elsewhere the plain update, bit for bit: the
 *                                               instance's schedule is not rewritten, its whole record and work record become candidate 0's)
 *   (run_num + 1) % gait_opt_freq == 0        : MPC::GetRealTimeUpdate, then MPCController::GaitOpt (gradient + LP)
 *   otherwise                                 : MPC::GetRealTimeUpdate
 * Asynchronous on the batch's stream; srbm_synchronize(h) to wait. */
int srbm_gait_rti_advance(srbm_gait* g, int first_run_num, int steps, int gait_opt_freq);
/* The same loop CLOSED over the plant of srbm_closed_loop_advance (controllers/mpc_controller.cpp:286-399: measured state in, one of the three
 * branches, out): for run r = first_run_num + i, r >= 1, t = r*dt (with srbm_plant_set_period: t = (r - 1)*p + p and "dt" below is p, per instance)
 *   plant:      exactly iteration r - 1 of srbm_closed_loop_advance -- integrate from t - dt to t under the current trajectory (substeps,
 *               advance_time as there), the instance's push if t - dt < push_time <= t, then (plant state, t, foot locations of the current
 *               trajectory at t) to the solve;
 *   controller: exactly the branch of srbm_gait_rti_advance on r -- r % freq == 0: line search for the instances whose gradient is ready, the
 *               plain update (zero-step candidates) for the others; (r + 1) % freq == 0: an RTI taken to the gap criterion whatever the batch's step
 *               rule says, then gradient and LP, ready := valid && lp_status == 0; otherwise a plain RTI, ready := 0.
 * MPC::AdjustForCurrentContacts (mpc_controller.cpp:312) is left out, as in srbm_closed_loop_advance: the plant has no contact model, its
 * "measured" contacts would be the plan's own.  A maximal stretch of plain runs is one multi-step plant launch (both launch forms of
 * srbm_rti_advance); with gait_opt_freq larger than the last run number the entry is bitwise srbm_closed_loop_advance(h, first_run_num - 1, steps, ..).
 * Refused, with nothing launched: no plant state set, first_run_num < 1, steps < 0, gait_opt_freq <= 0, substeps < 1, a step log without room
 * for `steps` records.  With a log enabled every run writes one record per instance: fields 0..57 as in the table above -- on a line-search run of
 * a ready instance 0 and 2..16 are still those of the instance's own last solve (only the winner's TRAJECTORY is installed, as
 * MPC::SetWarmStartTrajectory does), 1 is t, 17..41 the inputs from the plant, 42..57 evaluated on the installed trajectory -- and 58..63 the
 * outcome of the gait step.  Asynchronous on the batch's stream; srbm_synchronize(h) to wait. */
int srbm_gait_closed_loop_advance(srbm_gait* g, int first_run_num, int steps, int gait_opt_freq, int substeps, int advance_time);
/* imin[batch], costs[batch][10] of the LAST line search, whichever entry ran it (srbm_gait_line_search returns them itself; the advance entries
 * keep them on the device).  imin = -1 for an instance that was not ready and took the plain update.  Either pointer may be NULL. */
int srbm_gait_get_line_search_result(srbm_gait* g, int* imin, double* costs);
/* solver status / error bits of the candidates of the last line search: status[batch*10], err[batch*10] */
int srbm_gait_get_candidate_status(srbm_gait* g, int* status, int* err);
/* test hook: the candidate batch of the last line search (borrowed: never destroy it), candidate c of instance b at b * 10 + c; for the
 * read-back entries (srbm_get_status, srbm_get_sizes, srbm_export_qp) */
srbm_batch* srbm_gait_debug_candidates(srbm_gait* g);

/* ---- trajectory -> whole-body targets: the step right downstream of the MPC in the reference's
 * controller.  q = [base position (3), base quaternion xyzw (4), 12 joint angles in pinocchio's model order FL FR RL RR x
 * (hip, thigh, calf)]; v = [base linear, base angular velocity (base frame), 12 joint rates]. ---- */
/* leg geometry (what the reference reads from the URDF through pinocchio): per leg FL FR RL RR the origins of the hip joint in
 * the trunk, the thigh joint in the hip, the calf joint in the thigh and the foot in the calf; joint axes x, y, y, no rotation in
 * the origins (A1: models/a1_description/urdf/a1.urdf:363-466) */
typedef struct srbm_leg_kinematics { double origin[4][4][3]; } srbm_leg_kinematics;
int srbm_set_leg_kinematics(srbm_batch* h, const srbm_leg_kinematics* legs);
/* SingleRigidBodyModel::GetEndEffectorLocations (mpc/models/single_rigid_body_model.cpp:443-455): q[batch][19] -> ee[batch][4][3] */
int srbm_forward_kinematics(srbm_batch* h, const double* q, double* ee);
/* SingleRigidBodyModel::InverseKinematics (mpc/models/single_rigid_body_model.cpp:314-425): damped least squares on (foot position,
 * base pose), one foot after the other, eps 5e-6, step 0.1, <= 1000 iterations per foot.  state[batch][13] (base pose from it),
 * ee[batch][4][3] desired foot positions, q_guess[batch][19] (joint part used) -> q_out[batch][19]; iters[batch][4] and
 * status[batch] (0 converged, 1 not converged: the reference throws "IK did not converge.") may be NULL */
int srbm_inverse_kinematics(srbm_batch* h, const double* state, const double* ee, const double* q_guess, double* q_out, int* iters, int* status);
/* MPCController::GetTargetsFromTraj (controllers/mpc_controller.cpp:414-511) on the CURRENT trajectory of every instance at time[batch]:
 * interpolated state -> IK at `time` and `time + dt` -> q_des (in: the previous q_des as the IK guess, out), v_des[batch][18],
 * force_des[batch][4][3] = Trajectory::GetForce(ee, time).  status[batch]: 0 ok, 1 IK not converged, 2 time outside the trajectory
 * ("bad interp." / spline range: the reference throws) */
int srbm_get_targets_from_traj(srbm_batch* h, const double* time, double* q_des, double* v_des, double* force_des, int* status);
/* ... on device pointers (same shapes): ONE launch on the batch's stream, no copy, no synchronisation */
int srbm_get_targets_from_traj_dev(srbm_batch* h, const double* time_dev, double* q_des_dev, double* v_des_dev, double* force_des_dev, int* status_dev);

/* QPControl (controllers/qp_control.cpp): the 1 kHz whole-body inverse-dynamics QP, for every instance of the batch.
 * Model: the rigid bodies pinocchio builds from the URDF -- trunk, then FL FR RL RR x (hip, thigh, calf), links on fixed joints
 * merged into their parent -- each with mass, centre of mass and rotational inertia about it (row-major 3x3) in the frame of
 * its joint; gains and weights as the QPControl constructor takes them (qp_control.cpp:20-52: base_pos_gains = {kv, kp}, ...) */
typedef struct srbm_wbc_model {
    double body_mass[13], body_com[13][3], body_inertia[13][9];
    double torque_bounds[12], kp_joint_gains[12], kd_joint_gains[12];
    double base_pos_gains[2], base_ang_gains[2];
    double leg_tracking_weight, torso_tracking_weight, force_tracking_weight, friction_coef, max_grf;
} srbm_wbc_model;
int srbm_set_wbc_model(srbm_batch* h, const srbm_wbc_model* model);
/* QPControl::ComputeControlAction (qp_control.cpp:74-135) with the targets of UpdateTargetConfig / Vel / ForceTargets:
 * q[batch][19], v[batch][18] measured; contact[batch][4] (0/1: in contact, measured and desired); q_des[batch][19], v_des[batch][18],
 * force_des[batch][12] = 3 per foot IN CONTACT, stacked in foot order (the reference's force_target_).
 * control[batch][36] = joint position targets (12), joint velocity targets (12), torques (12) -- all zero where the QP failed, as the
 * reference returns; qp_sol[batch][30] = accelerations (18) then contact forces; status[batch] = SolveQuality | iterations << 8.
 * qp_dump (may be NULL): the assembled QP in the reference's layout per instance: A[50][30], lb[50], ub[50], diag P[30], w[30].
 * The solver relies on the rows being the controller's (every torque row and every contact-force row two-sided): with a torque bound or max_grf of
 * exactly zero such a row is an equality, and the instance is reported with status 8 (SRBM_OTHER) and a zero control action. */
int srbm_qp_control(srbm_batch* h, const double* q, const double* v, const int* contact, const double* q_des, const double* v_des,
                    const double* force_des, double* control, double* qp_sol, int* status, double* qp_dump);
/* ... on device pointers: control_dev[batch][36], qp_sol_dev[batch][30], status_dev[batch]; one launch, no copy, no synchronisation */
int srbm_qp_control_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const int* contact_dev, const double* q_des_dev, const double* v_des_dev,
                        const double* force_des_dev, double* control_dev, double* qp_sol_dev, int* status_dev);

/* ---- the control tick as ONE entry: MPCController::ComputeControlAction (controllers/mpc_controller.cpp:120-227) for every instance, with the
 * controller's member state q_des_ / v_des_ held by the batch.  = ReconstructState (:229-271) and GetEndEffectorLocations of the measured (q, v),
 * GetTargetsFromTraj, Trajectory::GetDesiredContacts(time), force_target_ stacked from GetForce (:181-188), QPControl::ComputeControlAction:
 * bit for bit what srbm_get_targets_from_traj -> srbm_eval_trajectory -> (stacking by the caller) -> srbm_qp_control give.
 * MEASURED CONTACTS ARE NOT AN ARGUMENT: the reference overwrites in_contact_ with the trajectory's (:172-173) and keeps only the contact frames. ---- */
/* MPCController's q_des_ (mpc_controller.cpp:206, set up in the constructor / InitSolver): q_des[batch][19], the IK guess of the next tick.
 * Required once before the first tick. */
int srbm_control_tick_reset(srbm_batch* h, const double* q_des);
/* q[batch][19], v[batch][18] measured; time[batch].
 * control[batch][36], qp_sol[batch][30] as srbm_qp_control; status[batch][2] = {targets status 0 / 1 / 2 as srbm_get_targets_from_traj,
 * QP status | iterations << 8}.  Each of the following may be NULL: q_des[batch][19], v_des[batch][18] (the targets: q_des_, v_des_ after the
 * tick), contact[batch][4] (Trajectory::GetDesiredContacts(time)), state[batch][13] (ReconstructState(q, v)), ee[batch][4][3]
 * (GetEndEffectorLocations(q)) -- the last two are what :142-156 publishes to the MPC thread, in the layout srbm_get_real_time_update[_dev] takes.
 * Targets status 1 (IK not converged): the QP runs on the q_des the IK left, as the chain of the single entries does.
 * Targets status 2 (the reference throws): zero control action, zero qp_sol, QP status 8, and the batch's q_des of that instance stays as it was.
 * q_des / v_des / contact are then what the targets step left -- for a time beyond the horizon: the q_des handed in, zero v_des, no contact.
 * The instance records are only read: lookup errors are NOT added to the error bits of srbm_get_status (srbm_eval_trajectory adds them).
 * Fails, before anything is staged or launched, without leg kinematics, whole-body model or srbm_control_tick_reset.  A clone carries q_des. */
int srbm_control_tick(srbm_batch* h, const double* q, const double* v, const double* time, double* control, double* qp_sol, int* status, double* q_des,
                      double* v_des, int* contact, double* state, double* ee);
/* ... on device pointers (same shapes, same optional ones): two launches on the batch's stream, no copy, no synchronisation */
int srbm_control_tick_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* time_dev, double* control_dev, double* qp_sol_dev, int* status_dev,
                          double* q_des_dev, double* v_des_dev, int* contact_dev, double* state_dev, double* ee_dev);

/* ---- whole-controller rollouts: MPC updates, control ticks and a whole-body plant, device-resident ----
 * The reference's top-level program (test/simulation_mpc.cpp:186-215) runs MPCController::ComputeControlAction at the control rate, an MPC update
 * whenever a newer state sample is there, and a whole-body simulation (MuJoCo: out of scope) in between.  srbm_controller_advance runs that loop for
 * every instance with a plant that needs no contact solver.  The whole-body QP (controllers/qp_control.cpp) holds the six floating-base rows of
 * M a + C v + g = S' tau + Js' F as equalities (:181-196), the stance-foot rows Js a = -Jsdot v as equalities (:198-222), and the joint rows of the
 * same equation, which define the torques it returns (:224-240, RecoverControlInputs :404-415): (a, F) of a solved QP IS the forward dynamics of the
 * whole-body model under the returned feed-forward torques with the planned stance feet held by the contact forces.  The plant integrates that a.
 * What the plant is NOT: it has no ground and no collision -- a foot is in stance when the plan says so, wherever it is (hence the foot heights in
 * the tick log); it does not model the joint PD loop the reference's robot adds to the feed-forward torque; and there is no
 * AdjustForCurrentContacts, for the same reason as in the other closed loops.
 *
 * The plant step of tick k, period h = tick_dt, t_k = k * h (one rounded product, never accumulated):
 *     a   = qp_sol[0..18) of the tick; 0 (the plant coasts) for exactly the instances to which the tick returned a zero control action
 *           (QP status > 1: not solved, or targets status 2)
 *     v+  = v + h a, then, if t_k < push_time <= t_k + h for the instance's push {time, impulse[6]} (srbm_plant_set_push):
 *           v+[0..3) += impulse[0..3) / mass, v+[3..6) += Ir^-1 impulse[3..6) with the instance's own mass and inertia, so that
 *           ReconstructState sees the momentum move by the impulse
 *     q+  = pinocchio::integrate(q, v+, h)
 * srbm_wb_plant_set_state: q[batch][19], v[batch][18]; allocates what the batch holds for the loop.  srbm_wb_plant_get_state: either pointer may be
 * NULL.  srbm_wb_plant_step_dev: the same kernel on the caller's device arrays q_dev[batch][19], v_dev[batch][18], in place, from qp_sol_dev[batch][30]
 * and status_dev[batch][2] as srbm_control_tick_dev returned them; one launch on the batch's stream, no copy, no synchronisation; never logs (a
 * host can drive the loop itself and be compared bit for bit).  srbm_batch_clone carries the plant's (q, v). */
int srbm_wb_plant_set_state(srbm_batch* h, const double* q, const double* v);
int srbm_wb_plant_get_state(srbm_batch* h, double* q, double* v);
int srbm_wb_plant_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, const double* qp_sol_dev, const int* status_dev);
/* Asynchronous on the batch's stream.  For k = first_tick .. first_tick + ticks - 1, in order:
 *   1. srbm_control_tick_dev on the batch's (q, v) at t_k, on the current trajectories;
 *   2. the plant step, and the record of the tick if a tick log is enabled;
 *   3. if k > 0 and k % ticks_per_update == 0: srbm_get_real_time_update_dev on the state and ee that step 1 wrote, at init_time = t_k.  The new
 *      trajectories are in force from tick k + 1 on: ComputeControlAction publishes (mpc_controller.cpp:142-156), the MPC thread picks up, with zero
 *      computation delay -- unless a latency is set (srbm_controller_set_latency, below: the ticks then read the PUBLISHED trajectories, which follow
 *      the MPC's by the latency of each instance).  With a step log enabled that solve writes its usual record, so srbm_rollout_summary_fold works on such a rollout unchanged.
 * The MPC period ticks_per_update * tick_dt is batch-wide and may lie off the node grid (as srbm_plant_set_period established).
 * Refused with a message, nothing launched, plant, trajectories, q_des and both log cursors untouched: no plant state set; no leg kinematics; no
 * whole-body model; no srbm_control_tick_reset; first_tick < 0; ticks < 0; ticks_per_update < 1; tick_dt not finite or <= 0;
 * ticks_per_update * tick_dt >= num_nodes * dt; a tick log or a step log without room. */
int srbm_controller_advance(srbm_batch* h, int first_tick, int ticks, int ticks_per_update, double tick_dt);
/* The tick log: log[slot][batch][SRBM_TICK_LOG_DOUBLES], one record per tick and instance, written by the plant-step kernel (the unlogged kernel
 * carries none of it); integers stored as doubles.  Every field is an output of THIS tick, read before the plant step: a record is, bit for bit,
 * what a one-tick call returns.
 *     index     content
 *     0, 1      tick index k, time t_k
 *     2         targets status
 *     3, 4      QP status, QP iterations
 *     5         flags: bit 0 the push was applied in this tick, bit 1 an MPC update followed this tick, bit 2 the plant coasted (plant kind 0
 *               only: the torque-driven plant never coasts on a zero control action), bit 3 a factorisation of the torque-driven plant broke down
 *     6..12     base position and quaternion of the plant's q
 *     13..18    base twist of the plant's v
 *     19..30    torques (control[24..36))
 *     31..42    contact forces per foot [4][3], unstacked from qp_sol, zero for a foot not in contact
 *     43..46    desired contacts [4]
 *     47..50    foot heights (ee[.][2]) [4]
 *     51..56    base acceleration a[0..6)
 *     57..63    plant kind 0: 0.  Plant kind 1 (the torque-driven plant, below), 58..62 from the LAST sub-step of the tick:
 *       57      the plant kind (1)
 *       58      number of joints whose torque was clamped
 *       59      max_j |tau_j - tau_ff,j|: what the PD loop and the limits changed
 *       60      the smallest vertical plant force over the stance feet, 0 with none; negative: the held foot pulls (the plant's stated limit
 *               without a ground)
 *       61      |a_plant - a_QP|_inf over the 18 accelerations
 *       62      |F_plant - F_QP|_inf over the stance feet
 *       63      0
 *     Plant kind 1 with a ground set (srbm_wb_plant_set_ground, below), 58..63 from the LAST sub-step of the tick: 57..59 as above, and
 *       60      the smallest vertical ground force over the feet the plan holds in stance, 0 if it holds none; >= 0 by construction (with a terrain
 *               in force, srbm_wb_plant_set_terrain: the smallest NORMAL force)
 *       61      |a_plant - a_QP|_inf over the 18 accelerations
 *       62      |F_ground - F_QP|_inf over all four feet, the QP's force zero for a foot out of the plan (as in fields 31..42)
 *       63      4096 + word.  Bit i: foot i in ground contact; bit 4 + i: foot i slipping; bit 8 + i: the plan's contact flag of foot i
 *               (field 43 + i) differs from the ground's
 *     Fields 31..42 and 51..56 are the QP's forces and acceleration for either kind.
 *     With sensors set (srbm_controller_set_sensors, below) the log keeps holding the truth: fields 6..18 are the plant's (q, v), not the measurement
 *     the tick read, which is what lets srbm_tick_summary_fold judge a fall and not an estimate of one.  Fields 47..50 come from the tick's ee and are
 *     therefore the feet of the measured q; every other field of 0..56 is an output of the tick that read the measurement.
 * The entries have the semantics of their srbm_step_log_* counterparts: srbm_tick_log_enable allocates max_ticks x batch records and sets the cursor to
 * 0 (0 disables and frees); capacity is checked before anything is launched; get (host, synchronous) and copy_dev (on the stream) fail for a slot
 * range outside [0, ticks_logged) and when no log is enabled.  A clone has logging off. */
#define SRBM_TICK_LOG_DOUBLES 64
int srbm_tick_log_record_doubles(void);                          /* SRBM_TICK_LOG_DOUBLES; callable without a GPU */
int srbm_tick_log_enable(srbm_batch* h, int max_ticks);
int srbm_tick_log_reset(srbm_batch* h);                          /* cursor 0, buffer kept */
int srbm_tick_log_count(srbm_batch* h, int* ticks_logged);
int srbm_tick_log_get(srbm_batch* h, int first_slot, int count, double* out);
int srbm_tick_log_copy_dev(srbm_batch* h, int first_slot, int count, double* out_dev);

/* ---- tick summaries: the tick log folded into one outcome record per instance, on the device ----
 * The tick-level counterpart of the rollout summaries above, which fold the step log (in a whole-controller rollout: one record per MPC update).
 * What only the tick log holds -- the torques, a held foot that pulls, clamped joints, slipping feet, the plan against the ground -- without copying
 * 512 bytes per tick and instance to the host.  The fold is INCREMENTAL in the same way: log a chunk of ticks, srbm_tick_summary_fold,
 * srbm_tick_log_reset, repeat; a rollout of any length needs a tick log of one chunk, and the summaries are bit for bit independent of the chunking
 * (every sum is accumulated in slot order).  The entries only read the log: no result changes.
 *
 * criteria[8], one set for the batch; ref[batch][6] = {p_ref[3], v_ref[3]} per instance, v_ref a linear velocity of the base.  R is a tick record
 * (the layout above).  Deviations are squared and the tilt is measured as u = 2 (qx qx + qy qy) = 1 - cos(tilt), qx = R[9], qy = R[10]: the fold
 * uses no division, square root or transcendental.
 *     0  z_min        fallen if p_z < z_min, p_z = R[8]
 *     1  tilt_max     fallen if u > tilt_max
 *     2  r2_settle    in band needs d2 = dx dx + dy dy <= r2_settle, dx = R[6] - ref_x, dy = R[7] - ref_y
 *     3  dz_settle    in band needs |p_z - ref_z| <= dz_settle
 *     4  tilt_settle  in band needs u <= tilt_settle
 *     5  v2_settle    in band needs |R[13..15] - v_ref|^2 <= v2_settle
 *     6, 7            reserved, must be 0
 * A record is in band when all four conditions hold.  A comparison with a NaN is false: a NaN never becomes a maximum or a minimum.
 *
 * One summary T, SRBM_TICK_SUMMARY_DOUBLES doubles, integers stored as doubles.  k is the 0-based ordinal of a record among those folded since the
 * last reset.  After a reset: counts and sums 0, every maximum -inf, every minimum +inf, every ordinal and every carry -1.  Where two records tie,
 * the first keeps the ordinal.  A field read as a set of bits (R[5], R[63] - 4096) is truncated to an integer; one that holds no set of bits
 * (negative, 2^53 or more, NaN) has no bit set.
 *     0         records folded
 *     1, 2      tick index R[0] of the first and of the last record
 *     3, 4      time R[1] of the first and of the last record
 *     5, 6      count of targets status R[2] != 0; ordinal of the first such record
 *     7, 8      count of QP status R[3] > 1 (the tick returned a zero control action); ordinal of the first such record
 *     9, 10     sum and max of the QP iterations R[4]
 *     11, 12    count of records with bit 0 of the flags R[5] (the push was applied); ordinal of the LAST such record
 *     13..15    count of records with flags bit 1 (an MPC update followed), bit 2 (the plant coasted), bit 3 (a factorisation broke down)
 *     31        count of records with a NaN among R[6..62]: such a record is counted here and in 0..15, and takes no part in 16..30 and 32..61
 *     16, 17    min and max of p_z
 *     18, 19    max d2 and the ordinal of its first occurrence
 *     20, 21    max u and its ordinal
 *     22        max |R[13..15] - v_ref|^2, summed as (x x + y y) + z z
 *     23        max |R[16..18]|^2, summed in the same order
 *     24        ordinal of the first fallen record
 *     25        ordinal of the last record NOT in band
 *     26        count of in-band records
 *     27        max over records and joints of |R[19 + j]|, j = 0..11
 *     28        sum over records of e, e the twelve squared torques R[19 + j]^2 added in ascending j
 *     29        max of the QP's f_z over the feet (R[33], R[36], R[39], R[42])
 *     30        min foot height R[47 + i] over records and feet with desired contact R[43 + i] == 1
 *     32        count of records whose four desired-contact flags R[43..46] differ from those of the record folded before it (among the records that
 *               take part)
 *     33..36    the flags folded last: the carry; the first record that takes part sets it and counts no switch
 *     37..40    per foot, count of records with flag 1
 *     41        max foot height over records and feet with flag 0
 *     42        0
 *     43..50    of the records with plant kind R[57] == 1 only:
 *       43      their count
 *       44      count of those with clamped joints, R[58] > 0
 *       45      sum of R[58]
 *       46      max R[59]
 *       47      min R[60]
 *       48      count of those with R[60] < 0: a held foot pulls (without a ground, the reason to discard the run)
 *       49, 50  max R[61], max R[62]
 *     51..61    of the records with a ground word, 4096 <= R[63] < 8192, word = R[63] - 4096, only:
 *       51      their count
 *       52..55  per foot i, count of records with word bit i (ground contact)
 *       56      sum over records of the number of slip bits 4..7 set
 *       57      sum over records of the number of plan-against-ground bits 8..11 set
 *       58      count of records with bits 0..3 all clear (airborne)
 *       59      ordinal k of the first record with a slip bit
 *       60      count of records whose bits 0..3 differ from those of the ground record folded before it
 *       61      those four bits of the ground record folded last as a number 0..15: the carry; the first ground record sets it and counts no switch
 *     62, 63    0
 * Derived, as for the rollout summaries: "settled from" = field 25 + 1; an instance is SETTLED if field 24 < 0 and field 25 < field 0 - 1; it has
 * FALLEN if field 24 >= 0.
 *
 * One study record, SRBM_TICK_STUDY_DOUBLES doubles, of summaries[instances][64] taken in ascending instance order:
 *     0         instances
 *     1, 2      number fallen, number settled
 *     3         number with summary field 7 > 0
 *     4, 5      max (-1 where none is settled) and sum of "settled from" over the settled instances
 *     6, 7, 8   max of summary field 18, of field 20, of field 27
 *     9, 10     sum of summary field 9, of field 44
 *     11        number with summary field 48 > 0
 *     12..14    sum of summary field 56, of field 57, of field 15
 *     15        min of summary field 47
 *
 * The entries are those of the rollout summaries, on the tick log.  srbm_tick_summary_enable: criteria[8] and ref[batch][6]; allocates the summaries
 * and resets them; criteria == NULL disables them and frees the buffers.  srbm_tick_summary_fold folds the tick-log slots [first_slot, first_slot +
 * count), which must lie in [0, ticks_logged), asynchronously on the batch's stream: a logged srbm_controller_advance, a fold and srbm_tick_log_reset
 * need no host synchronisation between them.  srbm_tick_summary_fold_dev runs the same kernel on any device array log_dev[slots][batch][64] of tick
 * records (a host-driven chain, tests); it needs no tick log.  _get (synchronous), _copy_dev, srbm_tick_study (synchronous), srbm_tick_study_dev and
 * srbm_tick_summary_allgather_dev (declared with the multi-GPU entries below) are their srbm_rollout_* counterparts.  srbm_tick_fold_host and
 * srbm_tick_study_host run the same fold of one record and the same reduction compiled for the host, on host arrays: log[slots][batch][64],
 * summaries[batch][64] in and out (the caller sets them to the reset state above); no GPU, no batch.
 * Refused before anything is queued, the batch and the summaries untouched, srbm_last_error naming the case: no tick log enabled; no tick summary
 * enabled; a slot or instance range outside what exists; NULL where it is not allowed; a criterion that is not finite; a reserved criterion other
 * than 0.  A clone has tick summaries off, as it has logging off. */
#define SRBM_TICK_SUMMARY_DOUBLES 64
#define SRBM_TICK_CRITERIA_DOUBLES 8
#define SRBM_TICK_REF_DOUBLES 6
#define SRBM_TICK_STUDY_DOUBLES 16
int srbm_tick_summary_doubles(void);                           /* SRBM_TICK_SUMMARY_DOUBLES; callable without a GPU */
int srbm_tick_summary_enable(srbm_batch* h, const double* criteria, const double* ref);
int srbm_tick_summary_reset(srbm_batch* h);
int srbm_tick_summary_fold(srbm_batch* h, int first_slot, int count);
int srbm_tick_summary_fold_dev(srbm_batch* h, const double* log_dev, int slots, int first_slot, int count);
int srbm_tick_summary_get(srbm_batch* h, int first, int count, double* out);
int srbm_tick_summary_copy_dev(srbm_batch* h, double* out_dev);
int srbm_tick_study(srbm_batch* h, double* study);
int srbm_tick_study_dev(srbm_batch* h, const double* summaries_dev, int instances, double* study_dev);
int srbm_tick_fold_host(const double* log, int slots, int batch, int first_slot, int count, const double* criteria, const double* ref, double* summaries);
int srbm_tick_study_host(const double* summaries, int instances, double* study);

/* ---- the torque-driven whole-body plant ----
 * The plant above integrates the QP's own accelerations: the torques and joint targets of the control action act on nothing, and the robot is exactly
 * the controller's model.  The torque-driven plant (kind 1) takes the control action and computes its own accelerations, per sub-step of h / S
 * (S = substeps, h / S one rounded quotient) on the plant's current (q, v):
 *     tau_j = clamp(tau_ff,j + kp_j (q_des,j - q_j) + kd_j (v_des,j - v_j), +-torque_limit_j)     tau_ff = control[24..36), q_des = control[0..12),
 *             v_des = control[12..24) of the tick, held over its sub-steps; the PD terms on the current (q, v), as position and velocity actuators
 *             (the reference's robot: controllers/include/controller.h:62-73, the actuators before the motors)
 *     M a - Js' F = S' tau - C v - g,  Js a = -Jsdot v      the constrained forward dynamics of the floating-base model on the PLANT'S OWN bodies with
 *             the planned stance feet held: 18 + 3 nc unknowns, nc the feet in contact, F stacked in foot order as qp_sol has it; solved exactly
 *             (LDL' of the quasi-definite matrix, no regularisation)
 *     v <- v + (h / S) a,  q <- pinocchio::integrate(q, v, h / S)
 * The push rule is the tick's (t_k < push_time <= t_k + h), applied to the velocity after the LAST sub-step's velocity update and before its
 * configuration step (S = 1: the order of the other plant); the impulse keeps using the instance's mass and Ir^-1.
 * What it is NOT: no ground and no collision -- a held foot pulls when the dynamics ask for it (tick log field 60) --, no contact solver, no
 * AdjustForCurrentContacts.  Where it differs from kind 0: to an instance whose tick returned a zero control action the actuators are OFF (tau = 0,
 * no PD) and the plant still runs, so the robot goes limp; the kind-0 plant coasts.  A sub-step whose factorisation meets a pivot that is not finite
 * or has the wrong sign takes a = 0 (flags bit 3 of the tick): no NaN reaches (q, v).
 *
 * srbm_wb_plant_set_kind: the plant srbm_controller_advance launches; 0 the QP-acceleration plant (the default), 1 the torque-driven plant.
 * Refused: a kind outside {0, 1}. */
int srbm_wb_plant_set_kind(srbm_batch* h, int kind);
/* The actuators of the torque-driven plant, per instance: kp[batch][12], kd[batch][12], torque_limit[batch][12] (+inf: none), and the batch-wide
 * number of sub-steps per tick.  These are the ROBOT'S actuator gains (the reference keeps them in its MuJoCo XML), not the QP's acceleration-level
 * kp_joint_gains / kd_joint_gains.  Refused, naming the instance and joint: kp or kd negative or not finite; a limit that is NaN or < 0;
 * substeps < 1. */
int srbm_wb_plant_set_actuators(srbm_batch* h, const double* kp, const double* kd, const double* torque_limit, int substeps);
/* The plant's own bodies per instance, in the layout of srbm_wbc_model: body_mass[batch][13], body_com[batch][13][3], body_inertia[batch][13][9].
 * Never called: the plant uses the controller's bodies (srbm_set_wbc_model).  One batch can so sweep a payload or inertia error.  Refused, naming the
 * instance and body: a mass <= 0, an entry that is not finite. */
int srbm_wb_plant_set_bodies_each(srbm_batch* h, const double* body_mass, const double* body_com, const double* body_inertia);
/* The solve alone on the plant's bodies: q[batch][19], v[batch][18], tau[batch][12], contact[batch][4] -> sol[batch][30] = a[18] then F stacked in
 * foot order (0 past 18 + 3 nc), status[batch] (may be NULL) 0, or 1 for a factorisation breakdown (sol is then 0).  Refused without leg kinematics
 * and without bodies (neither a whole-body model nor the plant's own). */
int srbm_wb_forward_dynamics(srbm_batch* h, const double* q, const double* v, const double* tau, const int* contact, double* sol, int* status);
/* ... on device pointers: one launch on the batch's stream, no copy, no synchronisation */
int srbm_wb_forward_dynamics_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* tau_dev, const int* contact_dev, double* sol_dev,
                                 int* status_dev);
/* The torque-driven plant step of tick `tick` on the caller's device arrays, the counterpart of srbm_wb_plant_step_dev: q_dev[batch][19],
 * v_dev[batch][18] in place from control_dev[batch][36], contact_dev[batch][4], status_dev[batch][2] as srbm_control_tick_dev returned them;
 * sol_dev (may be NULL) [batch][30] <- (a, F) of the last sub-step.  One launch on the batch's stream, no copy, no synchronisation; never logs (a
 * host can drive the loop itself and be compared bit for bit).  Refused without actuators, leg kinematics or bodies.
 * srbm_controller_advance launches this kernel instead of the QP-acceleration plant's when the kind is 1 (refused then without actuators); nothing
 * else in it changes.  srbm_batch_clone carries the kind, the actuators, the sub-steps and the bodies. */
int srbm_wb_fd_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, const double* control_dev, const int* contact_dev,
                        const int* status_dev, double* sol_dev);

/* ---- a compliant ground for the torque-driven plant ----
 * The torque-driven plant above holds the PLANNED stance feet wherever they are, and a held foot pulls.  A ground is a SETTING of plant kind 1 (not a
 * kind of its own): with one set the plant holds no foot.  Each foot meets a horizontal plane per instance that pushes and never pulls, with
 * stick / slip Coulomb friction, found from the plant's own foot positions.  ground[batch][8] per instance:
 *     0  ground height z0             finite, or -inf: no ground for this instance
 *     1  normal stiffness k_n         > 0             2  normal damping d_n          >= 0
 *     3  friction coefficient mu      >= 0
 *     4  tangential stiffness k_t     > 0             5  tangential damping d_t      >= 0
 *     6, 7  reserved                  must be 0
 * The contact state cs[batch][12] holds per foot {in_contact (0 | 1), anchor_x, anchor_y}.  Per sub-step of h / S on the plant's current (q, v):
 *     tau          the torque law of kind 1, unchanged (actuators off for a zero control action)
 *     p_i, w_i     foot i: world position from the forward kinematics of q (the batch's leg geometry), world velocity w_i = J_i v with the
 *                  LOCAL_WORLD_ALIGNED linear Jacobian J_i
 *     delta = z0 - p_z
 *     if !(delta > 0):  F_i = 0, in_contact = 0, anchor = (0, 0)
 *     else:  if the foot was not in contact after the previous sub-step: anchor = (p_x, p_y)
 *            N   = max(0, k_n delta - d_n w_z)
 *            T0  = -k_t (p_xy - anchor) - d_t w_xy,   lim = mu N,   n0 = sqrt(T0x^2 + T0y^2)
 *            n0 <= lim:  T = T0                        (stick)
 *            else:       T = (lim / n0) T0             (slip),  anchor = p_xy + (T + d_t w_xy) / k_t
 *            F_i = (T_x, T_y, N), in_contact = 1
 *     M a = S' tau - C v - g + sum_i J_i' F_i          on the plant's own bodies: 18 unknowns, no constraint rows, solved exactly (LDL' of M)
 *     v <- v + (h / S) a,  q <- pinocchio::integrate(q, v, h / S);  the push where kind 1 applies it
 * cs is carried from sub-step to sub-step and, in the batch, from tick to tick.  A sub-step whose factorisation meets a pivot that is not finite or not
 * positive takes a = 0 and reports (a, F) = 0 (flags bit 3 of the tick); its contact state is what the law left.
 * What it is NOT: compliant, not rigid (a foot that carries N sinks by N / k_n); no impact law; no LCP; one horizontal plane per instance
 * (sloped patches with a friction coefficient each: srbm_wb_plant_set_terrain, below).  The plan is told of the ground's contacts only with srbm_controller_set_contact_feedback on (below: MPC::AdjustForCurrentContacts before
 * every MPC update); off, the default, the controller keeps believing its plan.  Tick log fields 43..46 against field 63 show where the plan and the
 * ground disagree.
 *
 * srbm_wb_plant_set_ground: ground[batch][8]; NULL removes the ground, kind 1 is then the held-feet plant again.  Kind 0 ignores a ground.  Refused,
 * naming the instance and the field, the batch untouched: a field that is not finite (z0 may be -inf) or outside its range; a reserved field != 0.
 * srbm_wb_plant_get_contact_state / _set_contact_state: cs[batch][12] of the batch (after srbm_wb_plant_set_state, which resets it to "no foot in
 * contact"); set refuses an in_contact other than 0 or 1 and an anchor that is not finite.  srbm_batch_clone carries the ground and the contact state. */
int srbm_wb_plant_set_ground(srbm_batch* h, const double* ground);
int srbm_wb_plant_get_contact_state(srbm_batch* h, double* cs);
int srbm_wb_plant_set_contact_state(srbm_batch* h, const double* cs);
/* The law and the solve alone: q[batch][19], v[batch][18], tau[batch][12], cs_in[batch][12] -> sol[batch][30] = a[18] then F[4][3] in foot order, zero
 * for a foot in the air; cs_out[batch][12]; status[batch] (may be NULL) 0, or 1 for a factorisation breakdown (sol is then 0).  Refused without a
 * ground, leg kinematics or bodies. */
int srbm_wb_ground_dynamics(srbm_batch* h, const double* q, const double* v, const double* tau, const double* cs_in, double* sol, double* cs_out, int* status);
/* ... on device pointers: one launch on the batch's stream, no copy, no synchronisation */
int srbm_wb_ground_dynamics_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* tau_dev, const double* cs_in_dev, double* sol_dev,
                                double* cs_out_dev, int* status_dev);
/* The ground step of tick `tick` on the caller's device arrays, the counterpart of srbm_wb_fd_step_dev: q_dev[batch][19], v_dev[batch][18],
 * cs_dev[batch][12] in place from control_dev[batch][36] and status_dev[batch][2] as srbm_control_tick_dev returned them (the plan's contact flags
 * are not an input); sol_dev (may be NULL) [batch][30] <- (a, F) of the last sub-step.  One launch on the batch's stream; never logs.  Refused
 * without a ground, actuators, leg kinematics or bodies.
 * srbm_controller_advance launches this kernel on the batch's (q, v, cs) when the kind is 1 and a ground is set; nothing else in it changes. */
int srbm_wb_ground_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, double* cs_dev, const double* control_dev,
                            const int* status_dev, double* sol_dev);

/* ---- a terrain for that ground: sloped patches, friction per patch ----
 * A terrain is a SETTING of the ground, as the ground is a setting of plant kind 1: a list of rectangular patches per instance, each with a plane
 * of its own and a friction coefficient of its own.  Contact is resolved along the patch normal, friction acts in the patch's tangent plane.
 * terrain[batch][n_patches][8], 1 <= n_patches <= SRBM_TERRAIN_PATCHES, per patch:
 *     0..3  x_min, x_max, y_min, y_max   the rectangle in world x, y; may be -inf / +inf; x_min > x_max: the patch is empty (how an instance uses
 *                                        fewer patches than the batch)
 *     4     z0                           finite: the surface is z = z0 + gx x + gy y in world coordinates, through the world origin (no reference
 *     5, 6  gx, gy                       finite   point, so an unbounded patch is well defined)
 *     7     mu                           finite, >= 0
 * The unit normal n = (nx, ny, nz) of a patch is formed once, when the terrain is set, in double: s = sqrt((1 + gx gx) + gy gy), nx = -gx / s,
 * ny = -gy / s, nz = 1 / s.  The ground's k_n, d_n, k_t, d_t (ground[b][1, 2, 4, 5]) stay the compliance of every patch and ground[b][0] = -inf still
 * means "nothing under this instance"; with a terrain set the ground's own z0 (other than as that switch) and mu are not used.
 * The contact state keeps its shape cs[batch][12]; with a terrain in_contact holds 1 + j, j the patch the foot is on, instead of 1 (every reader
 * tests != 0: contact feedback, the word of tick log field 63).  The stored patch number is only ever compared, never used as an index.
 * Per sub-step and foot i, p and w = J_i v as on the ground; every line is one rounded operation, sums associate as written:
 *     j = the LAST patch t with x_min <= p.x <= x_max and y_min <= p.y <= y_max (later patches lie over earlier ones); none: air
 *     hx = gx p.x; hy = gy p.y; h0 = z0 + hx; zp = h0 + hy; dz = zp - p.z; delta = nz dz
 *     !(delta > 0): air  ->  F = 0, in_contact = 0, anchor = (0, 0)
 *     first = (in_contact after the previous sub-step) != 1 + j          (not in contact, or in contact with another patch: re-anchored)
 *     wn = (nx wx + ny wy) + nz wz;   wt = w - wn n
 *     ns = k_n delta; nd = d_n wn; n1 = ns - nd; N = fmax(0, n1)
 *     pb = p + delta n                                                    (the foot projected onto the surface)
 *     A  = pb if first, else (ax, ay, (z0 + gx ax) + gy ay)
 *     e  = p - A;  en = (nx ex + ny ey) + nz ez;  et = e - en n
 *     sv = k_t et; dv = d_t wt; T0 = -sv - dv;  lim = mu N;  nn = (T0x T0x + T0y T0y) + T0z T0z;  n0 = sqrt(nn)
 *     n0 <= lim:  T = T0,              anchor = (A.x, A.y)                (stick)
 *     else:       sc = lim / n0; T = sc T0; u = T + dv; qv = u / k_t; anchor = (pb.x + qv.x, pb.y + qv.y)     (slip)
 *     F = T + N n  (world components);  in_contact = 1 + j
 * then the ground's solve M a = S' tau - C v - g + sum_i J_i' F_i, its integration and its push, unchanged.  On one unbounded level patch,
 * n = (-0, -0, 1), every statement returns the bits of the plane's law: the terrain is that law generalised, not a second one.
 * The tick record with a terrain in force: fields 0..59, 61, 62 as on the ground (forces in world components); field 60 is the smallest NORMAL
 * force N over the feet the plan holds (today's value on a level patch; >= 0 by construction); field 63 has the ground's format 4096 + word, so the
 * tick summaries fold terrain rollouts unchanged.
 * What it is NOT: no side faces -- a foot that crosses the edge of a raised patch below its surface is at once delta deep in it and is pushed out
 * with k_n delta, so join levels with ramps or keep steps small; still compliant; no impact law; no edges, curvature or rolling contact; the
 * controller is told nothing of the terrain (contact feedback apart).
 *
 * srbm_wb_plant_set_terrain: NULL removes the terrain.  A terrain needs a ground: setting one without a ground is refused; removing the ground
 * removes nothing else, and the terrain is ignored while no ground is set or the kind is 0, as the ground is ignored under kind 0.  With kind 1, a
 * ground and a terrain all set, srbm_controller_advance, srbm_gait_controller_advance, srbm_wb_ground_dynamics[_dev] and srbm_wb_ground_step_dev run
 * the terrain's kernels (csrc/srbm_wb_terrain.hiph); they are to the terrain what they are to the ground.  Refused, naming instance, patch and field,
 * the batch untouched: NaN anywhere; z0, gx, gy, mu not finite; mu < 0; n_patches out of range.  While a terrain is set,
 * srbm_wb_plant_set_contact_state accepts the integers 0..n_patches for in_contact.  srbm_batch_clone carries the terrain. */
#define SRBM_TERRAIN_PATCHES 8
#define SRBM_TERRAIN_DOUBLES 8
int srbm_wb_plant_set_terrain(srbm_batch* h, const double* terrain, int n_patches);

/* ---- a joint model for the torque-driven plant: damping, rotor inertia, friction, range stops, motor lag ----
 * The torque law of kind 1 commands a torque that acts at once on a frictionless, massless, unbounded joint.  A joint model is a SETTING of plant
 * kind 1, per instance and per joint, off by default, on all three surfaces (held feet, ground, terrain).  joints[batch][12][8], the joints in this
 * library's order (control[0..12), q[7..19): FL, FR, RL, RR, each hip, thigh, calf), per joint:
 *     0  viscous damping b (N m s/rad)       >= 0
 *     1  armature I_a (kg m^2)               >= 0      the rotor's reflected inertia, added to the joint's diagonal entry of M
 *     2  dry friction f_c (N m)              >= 0
 *     3  stiction band v_s (rad/s)           > 0 where f_c > 0, else must be 0: the friction is f_c clamp(v / v_s, +-1)
 *     4, 5  q_min, q_max (rad)               finite, or -inf / +inf for none; q_min < q_max
 *     6  motor time constant T (s)           >= 0
 *     7  reserved                            must be 0
 * stops[batch][2] = {k_l > 0 (N m/rad), d_l >= 0 (N m s/rad)}: the compliance of every range stop of the instance.
 * The state of the model is the motor torque js[batch][12] = tau_m.  Per sub-step of hs = h / S and joint j, on the plant's current (q_j, v_j);
 * every line is one rounded operation, and a term whose coefficient is 0 is SKIPPED, with no arithmetic on it at all:
 *     cmd     the command of the torque law of kind 1 as it stands, the clamp to the torque limit included; 0 for an instance whose tick returned a
 *             zero control action (the actuators are off)
 *     T == 0: tau_m = cmd
 *     else:   d = cmd - tau_m; ad = alpha d; tau_m = tau_m + ad         s = T + hs; alpha = hs / s, formed once per launch (an "off" instance
 *                                                                       decays through its lag)
 *     t = tau_m
 *     b != 0:    pd = b v; t = t - pd
 *     f_c != 0:  r = v / v_s; r = fmin(fmax(r, -1), 1); pc = f_c r; t = t - pc
 *     e = q_min - q;  e > 0:  sl = k_l e; dl = d_l v; sl = sl - dl; sl = fmax(sl, 0); t = t + sl         (the lower stop)
 *     e = q - q_max;  e > 0:  su = k_l e; du = d_l v; su = su + du; su = fmax(su, 0); t = t - su         (the upper stop; a stop never pulls a
 *                                                                                                         joint towards itself, as the ground never pulls)
 *     t is the joint torque of the sub-step
 * and in the solve of the sub-step M[6 + j][6 + j] = M[6 + j][6 + j] + I_a where I_a != 0, before the factorisation (30 rows with the feet held, 18
 * on a ground or a terrain).  The transparent model -- b = I_a = f_c = v_s = T = 0 and infinite ranges -- therefore returns the bytes of the plant
 * without the setting.
 * The tick record keeps its fields: 58 counts the joints whose COMMAND was clamped, 59 is max |t - tau_ff| with the model's t; no field is added, and
 * the tick summaries fold such rollouts unchanged.  The model's own record jrec[batch][8], since the state was set:
 *     0  sub-steps run                        1  sub-steps with any joint beyond its range
 *     2  the largest excursion beyond a range (rad)
 *     3  the largest |pd + pc| (N m)          4  the largest |cmd - tau_m|, tau_m after the motor's statement (N m)
 *     5  bit mask (bit j: joint j) of the joints ever beyond their range, as a double        6, 7  0
 * What it is NOT: no command delay (the lag is first order); no torque-speed curve; no gear backlash; the friction is a regularised band, not a
 * constraint (a joint loaded below f_c creeps at v_s load / f_c); the stops are compliant (a joint passes its range by load / k_l).  The sub-step is
 * explicit: hs must resolve b / (I_link + I_a), f_c / (v_s (I_link + I_a)) and sqrt(k_l / (I_link + I_a)), I_link the link's own inertia about the
 * joint (DESIGN.md states the limits in numbers for the A1).
 *
 * srbm_wb_plant_set_joints: NULL joints removes the setting and frees its buffers.  Refused, naming instance, joint and field, the batch untouched: a
 * value that is not finite (other than q_min = -inf, q_max = +inf), a value outside its range, q_min >= q_max, a reserved entry that is not 0.  js
 * and jrec are zero when the setting is made; srbm_wb_plant_set_state resets both; srbm_batch_clone carries setting, state and record.  Kind 0
 * ignores the setting.  With kind 1 and a joint model set, srbm_controller_advance, srbm_gait_controller_advance and the three _step_dev entries
 * (srbm_wb_fd_step_dev, srbm_wb_ground_step_dev, on a terrain too) run the full law on the batch's js and jrec and advance them;
 * srbm_wb_forward_dynamics[_dev] and srbm_wb_ground_dynamics[_dev] take tau as the NET joint torque and add the armature, nothing else
 * (the kernels of csrc/srbm_wb_joints.hiph).
 * srbm_wb_plant_get_joints returns the setting; _get_joint_state / _set_joint_state read and write js (set refuses a value that is not finite);
 * _get_joint_record returns jrec.  All four are refused while no joint model is set.
 * srbm_joint_law_host: the same function the kernels compile, without a GPU, over recorded sub-steps: cmd, q_j, v_j [substeps][batch][12] are the
 * command after its clamp and the joint's angle and rate of each sub-step, off[batch] != 0 an instance with its actuators off (cmd is read as 0),
 * js_inout[batch][12] the motor torques before and after, tau_out[substeps][batch][12] <- t, jrec_inout (may be NULL) [batch][8] folded into. */
#define SRBM_JOINT_DOUBLES 8
#define SRBM_JOINT_STOP_DOUBLES 2
#define SRBM_JOINT_RECORD_DOUBLES 8
int srbm_wb_plant_set_joints(srbm_batch* h, const double* joints, const double* stops);
int srbm_wb_plant_get_joints(srbm_batch* h, double* joints, double* stops);
int srbm_wb_plant_get_joint_state(srbm_batch* h, double* js);
int srbm_wb_plant_set_joint_state(srbm_batch* h, const double* js);
int srbm_wb_plant_get_joint_record(srbm_batch* h, double* jrec);
int srbm_joint_law_host(int batch, int substeps, double h, const double* joints, const double* stops, const double* cmd, const int* off, const double* q_j,
                        const double* v_j, double* js_inout, double* tau_out, double* jrec_inout);

/* ---- timed external wrenches on any body of the torque-driven plant ----
 * The push above is one momentum impulse per instance, on the base, at one instant.  A wrench schedule is a SETTING of plant kind 1, per instance,
 * off by default, on all three surfaces (held feet, ground, terrain), with or without a joint model: a shove held for 150 ms, two pushes in one run,
 * a kick on a shank, a force off the trunk's origin that also turns the robot, a payload dropped on the back at t = 2 s.
 * wrenches[batch][n_events][16], 1 <= n_events <= SRBM_WRENCH_EVENTS, per event:
 *     0       t0, start (s)                  finite
 *     1       d, duration (s)                >= 0 or +inf; d == 0 is an EMPTY slot that never acts
 *     2       body                           integer 0..12 in SrbmWbcParams::body order: 0 trunk, 1 + 3 leg + k for hip / thigh / calf of FL FR RL RR
 *     3       frame of force and torque      0 world axes, 1 the body's axes (the wrench turns with the body)
 *     4..6    point r (m)                    in the body's joint frame, the frame SrbmBody::com is stated in
 *     7..9    force (N)                      finite
 *     10..12  torque (N m)                   finite
 *     13..15  reserved                       must be 0
 * The rule, every line one rounded operation.  In sub-step s of tick `tick` of period h with S sub-steps:
 *     hs = h / S;  p = (double)s hs;  ts = tk + p;  te = t0 + d;        event e is ACTIVE iff d != 0 && ts >= t0 && ts < te
 * with tk = tick h, so a rollout cut anywhere is the same rollout.  For an active event on body (ee, k), or on the trunk, with the kinematics of
 * the sub-step's q (R, origin: the rotation and the joint centre of the body, or the base's; Rb, pb the base's; ax, c the leg's joint axes and centres):
 *     x = origin + R r;   F, N the force and torque in world axes (rotated by R where the frame is 1)
 *     Q[jj] = colb . F;   Q[3 + jj] = (colb x (x - pb)) . F + colb . N                                  colb = column jj of Rb
 *     Q[6 + 3 ee + jj] = (ax[ee][jj] x (x - c[ee][jj])) . F + ax[ee][jj] . N     for jj <= k of that leg only;   Q = 0 in every other column
 * -- the stance Jacobian's column formulas with the point in the place of the foot -- the events summed in event order, one fma chain per column, and
 * b = b + Q on rows 0..17 of the sub-step's right-hand side after its existing statements.  A sub-step of an instance in which NO event is active
 * runs no arithmetic of the setting on (q, v) or on the right-hand side (no + 0.0 either): a schedule of empty slots, or of events outside the
 * rollout, returns the bytes of the plant without the setting.  The existing push is untouched and combines with the schedule.
 * The record wrec[batch][8], since the state was set:
 *     0  sub-steps run                        1  sub-steps with any event active
 *     2  bit mask (bit e: event e) of the events that ever acted, as a double
 *     3  the largest |Q|_inf
 *     4..6  the delivered linear impulse in world axes: the sum of hs F over the active (event, sub-step) pairs        7  0
 * The tick record keeps its fields; bit 4 (value 16) of its flags (field 5) is set when an event acted in any sub-step of the tick.
 * What it is NOT: a rectangular profile only; the force follows the body point but is no contact, so it has no friction and no geometry; an impulse
 * is a short event of one sub-step; the controller is told nothing; it is not applied under plant kind 0.
 *
 * srbm_wb_plant_set_wrenches: NULL wrenches removes the setting and frees its buffers.  Refused, naming instance, event and field, the batch
 * untouched: a NaN, a value that is not finite (other than d = +inf), d < 0, a body or a frame that is not an integer in range, a reserved entry
 * that is not 0; n_events out of range.  The record is zero when the setting is made; srbm_wb_plant_set_state zeroes it; srbm_batch_clone carries the
 * setting and the record.  Kind 0 ignores the setting, as it ignores the joint model.  With kind 1 and a schedule set, srbm_controller_advance,
 * srbm_gait_controller_advance and the three _step_dev entries apply it and advance the record (the kernels of csrc/srbm_wb_wrench.hiph).
 * srbm_wb_forward_dynamics[_dev] and srbm_wb_ground_dynamics[_dev] have no time and ignore the setting.
 * srbm_wb_plant_get_wrenches: *n_events and, where wrenches is not NULL, wrenches[batch][*n_events][16] as set; _get_wrench_record returns wrec.  Both
 * are refused while no schedule is set.
 * srbm_wb_wrench_force[_dev]: the generalized force alone, on the function the step compiles: Q_out[batch][18] of the events active at time[batch]
 * (a sub-step time ts) on q[batch][19], 0 where none is; mask_out[batch] bit e: event e is active.  Needs the leg geometry and a schedule.
 * srbm_wrench_active_host: the activity rule without a GPU: mask_out[ticks][substeps][batch] of ticks first_tick .. first_tick + ticks - 1. */
#define SRBM_WRENCH_EVENTS 8
#define SRBM_WRENCH_DOUBLES 16
#define SRBM_WRENCH_RECORD_DOUBLES 8
int srbm_wb_plant_set_wrenches(srbm_batch* h, const double* wrenches, int n_events);
int srbm_wb_plant_get_wrenches(srbm_batch* h, double* wrenches, int* n_events);
int srbm_wb_plant_get_wrench_record(srbm_batch* h, double* wrec);
int srbm_wb_wrench_force(srbm_batch* h, const double* time, const double* q, double* Q_out, int* mask_out);
int srbm_wb_wrench_force_dev(srbm_batch* h, const double* time_dev, const double* q_dev, double* Q_dev, int* mask_dev);
int srbm_wrench_active_host(int n_events, const double* wrenches, int batch, int first_tick, int ticks, double tick_dt, int substeps, int* mask_out);

/* ---- the MPC update of the rollout in full: MPCController::MPCUpdate (controllers/mpc_controller.cpp:299-346) ----
 * Step 3 of srbm_controller_advance is MPC::GetRealTimeUpdate alone.  The reference's update does two more things, both off by default here.
 *
 * Contact feedback (replaces mpc_controller.cpp:322, mpc_.AdjustForCurrentContacts(time, contact) -> mpc/mpc.cpp:1195-1203): with the setting on,
 * every update tick k of srbm_controller_advance runs, between the control tick and the plant step, the rule of srbm_adjust_for_current_contacts on
 * the time array of the tick (t_k) and the batch's contact state cs: foot i counts as measured in contact iff cs[3 i] != 0.  At that point cs is the
 * ground's state after tick k - 1, the contact the reference's simulator measures at t_k and hands to ComputeControlAction
 * (simulation/simulation_robot.cpp:144-156).  A foot on the ground whose plan says swing and whose planned touch-down is less than 70 ms away has
 * that touch-down moved to t_k; the error bits are those of srbm_adjust_for_current_contacts (64 where the reference throws).  The control tick of
 * tick k has read the old knot tables, the plant step reads none: the new schedule is in force from the update on.  One launch on the batch's
 * stream, no copy, no synchronisation.  The tick log and the step log keep their layouts (the measured flags at t_k are field 63 bits 0..3 of the
 * record of tick k - 1).
 * srbm_controller_set_contact_feedback: on = 0 (the default) | 1.  With it on, srbm_controller_advance and srbm_gait_controller_advance are refused,
 * naming the setting, with the batch untouched, unless the plant is of kind 1 with a ground set: without a ground nothing measures a contact.
 * The feedback record fb[batch][8]: per foot {number of touch-downs moved, t of the last move (-1 if none)}; srbm_wb_plant_set_state resets it,
 * srbm_controller_get_contact_feedback reads it (after the work queued so far).  srbm_batch_clone carries the setting and the record.
 * srbm_controller_contact_feedback_dev: the kernel alone on the caller's device arrays time_dev[batch], cs_dev[batch][12], for tests and host-driven
 * chains; it counts in fb the same way.  Refused before srbm_wb_plant_set_state (which allocates fb). */
int srbm_controller_set_contact_feedback(srbm_batch* h, int on);
int srbm_controller_get_contact_feedback(srbm_batch* h, double* fb);
int srbm_controller_contact_feedback_dev(srbm_batch* h, const double* time_dev, const double* cs_dev);
/* The gait step (replaces mpc_controller.cpp:324-346, the branch on the run number): srbm_controller_advance on the batch of `g` -- the same
 * loop, the same refusals, the same tick and plant launches, contact feedback before the update when it is on -- with the update after tick k,
 * run r = k / ticks_per_update (r >= 1), branched as srbm_gait_rti_advance branches on r, F = gait_opt_freq:
 *     r % F == 0          GaitOptimizer::LineSearch for the instances whose gradient is ready, the plain update (zero-step candidates) for the others
 *     (r + 1) % F == 0    an RTI taken to the gap criterion whatever the batch's step rule says, then gradient and LP; ready := valid && lp_status == 0
 *     otherwise           the plain update; ready := 0
 * on the state, time and ee of the tick, as srbm_get_real_time_update_dev takes them.  The ready flags live in `g` and r follows from k: a rollout
 * split into several calls is the same rollout.  With a step log enabled every update writes one record: plain runs as srbm_controller_advance
 * writes them, gradient and line-search runs with fields 58..63 as srbm_gait_closed_loop_advance writes them.  With F beyond the last run number the
 * entry is bitwise srbm_controller_advance.  Refused in addition: a NULL handle, gait_opt_freq <= 0.  The caller's own srbm_gait_compute_gradient /
 * _sensitivity after a rollout still refuse a last solve that ended by the step rule. */
int srbm_gait_controller_advance(srbm_gait* g, int first_tick, int ticks, int ticks_per_update, double tick_dt, int gait_opt_freq);

/* ---- timed motion commands: the tracking target of a whole-controller rollout over time, per instance ----
 * The tracking target is one state_des12 per instance, set on the host (srbm_add_quadratic_tracking_cost[_each] stores w = -Q des,
 * srbm_set_linear_final_cost[_each] stores Phi_w) and constant for a launch: the reference's apps fix it at construction (apps/mpc_demo.cpp:62-64,
 * controllers/mpc_controller.cpp:64-67).  A command schedule is a SETTING of the rollout, per instance, off by default: "walk at 0.3 m/s for two
 * seconds, then stop" in one launch, a sweep of commanded speeds in one batch.
 * cmds[batch][n_events][28], 1 <= n_events <= SRBM_CMD_MAX_EVENTS, per event:
 *     0       t0 (s)                         finite, strictly ascending within an instance
 *     1       flags                          0, or 1: bit 0 = RELATIVE; no other bit
 *     2       lead (s)                       finite, >= 0
 *     3       reserved                       must be 0
 *     4..15   des12                          a tangent state in the layout of srbm_add_quadratic_tracking_cost, finite
 *     16..27  rate12                         a rate per tangent component, per second, finite
 * The rule (csrc/srbm_command.hiph), every line one rounded operation.  At the MPC update after tick k, at t = t_k, on the state the tick
 * reconstructed (with sensors on: from the measurement):
 *     the event IN FORCE is the last one with t0 <= t.  None: nothing of the instance is touched -- costs, state, record.
 *     dt = t - t0;  s = dt + lead;  p[i] = rate12[i] s;  des[i] = des12[i] + p[i]
 *     a relative event: the FIRST update at which it is in force latches (x, y) of that state as the anchor (command state);
 *         des[0] = des[0] + anchor x;  des[1] = des[1] + anchor y.       An absolute event adds nothing (no + 0.0).  Only x and y can be relative.
 *     w[i] = -1 * sum_j Q[12 i + j] des[j];   Phi_w[i] = -1 * sum_j Phi[12 i + j] des[j]      j ascending, products and sums rounded separately
 * -- the arithmetic of srbm_add_quadratic_tracking_cost, so that the setters called with des and -Phi des write the same bytes as the command.
 * One launch on the batch's stream before the update (after the contact feedback), no copy, no synchronisation.  It writes w and Phi_w of the
 * instance's record on the device and, under srbm_gait_controller_advance, of the records of its line-search candidates.  The host's costs are
 * NOT changed: whatever re-uploads the records (a cost setter, a tolerance) between two updates puts the base costs back, which is harmless inside
 * a rollout because the next update writes the command again; setting or removing the schedule does exactly that.
 * Command state cstate[batch][4]: index of the latched event (-1: none), anchor x, anchor y (0 for an absolute event), latch time.
 * Command record crec[batch][32]:
 *     0  updates at which an event was in force     1  index in force at the last of them (-1: none yet)     2  events begun     3  time of the last latch
 *     4, 5  the anchor     6  the largest horizontal distance, at an update, between the state's (x, y) and the UN-LED target
 *     des12 + rate12 (t - t0) (+ anchor)            7  the sum of the squares of that distance             8..19  the des last written     20..31  0
 * What it is NOT: there is ONE target for the whole horizon, and `lead` is the only look-ahead (no per-node reference); only x and y can be
 * relative; a rate on an orientation component advances the tangent coordinate linearly; the `ref` band of the rollout and tick summaries still
 * refers to a fixed target -- the tracking error against a moving target is fields 6 and 7 of this record.
 * Applied by srbm_controller_advance and srbm_gait_controller_advance alone.  srbm_rti_advance, srbm_closed_loop_advance, srbm_gait_rti_advance and
 * srbm_gait_closed_loop_advance IGNORE the setting.
 *
 * srbm_controller_set_commands: n_events = 0 (cmds may be NULL) removes the setting.  Refused before anything is staged, naming the entry, the
 * instance, the event and the field, with the setting in force untouched: a NULL handle, n_events outside 0..8, a value that is not finite, a t0
 * that does not ascend, a flag other than 0 or 1, a negative lead, a reserved double that is not 0.  State and record are zero with both indices -1
 * when the setting is made.  Setting and removing mark the records changed, so that the host's base costs are on the device before anything runs.
 * srbm_wb_plant_set_state re-initialises state and record; srbm_batch_clone carries setting, state and record.
 * srbm_controller_get_commands: *n_events (0: none set) and, where cmds is not NULL, cmds as set.  _get_command_state, _set_command_state (a latched
 * index -1 .. n_events - 1, finite values) and _get_command_record are refused while no schedule is set.
 * srbm_controller_get_command_costs: w[batch][12] and Phi_w[batch][12] of the records ON THE DEVICE after the work queued so far; without a
 * schedule they are the host's.  With a schedule set srbm_export_qp takes its linear costs from the same place.
 * srbm_controller_command_dev: the kernel alone on time_dev[batch], state_dev[batch][13], for host-driven chains, in the place it has in the
 * rollout: before srbm_get_real_time_update_dev.  It writes the batch's own records, not a gait handle's candidates.
 * srbm_command_target_host: the same rule without a GPU, for n_updates updates in turn: times[n_updates][batch], states13[n_updates][batch][13],
 * Q144 / Phi144[batch][144] -> des12, w12, Phi_w12 [n_updates][batch][12], NaN where no event is in force; cstate[batch][4] and crec[batch][32]
 * are folded into (initially {-1, 0, 0, 0} and zero with field 1 at -1). */
#define SRBM_CMD_MAX_EVENTS 8
#define SRBM_CMD_EVENT_DOUBLES 28
#define SRBM_CMD_STATE_DOUBLES 4
#define SRBM_CMD_REC_DOUBLES 32
int srbm_command_event_doubles(void);
int srbm_command_record_doubles(void);
int srbm_controller_set_commands(srbm_batch* h, const double* cmds, int n_events);
int srbm_controller_get_commands(srbm_batch* h, double* cmds, int* n_events);
int srbm_controller_get_command_state(srbm_batch* h, double* cstate);
int srbm_controller_set_command_state(srbm_batch* h, const double* cstate);
int srbm_controller_get_command_record(srbm_batch* h, double* crec);
int srbm_controller_get_command_costs(srbm_batch* h, double* w, double* Phi_w);
int srbm_controller_command_dev(srbm_batch* h, const double* time_dev, const double* state_dev);
int srbm_command_target_host(int n_events, const double* cmds, int batch, const double* Q144, const double* Phi144, int n_updates, const double* times,
                             const double* states13, double* cstate, double* des12, double* w12, double* Phi_w12, double* crec);

/* ---- MPC computation latency: the time between the start of an MPC update and the tick from which the control tick sees its result ----
 * The reference's MPC thread (controllers/mpc_controller.cpp:299-398) loops: newest state sample, solve, publish traj_, again; ComputeControlAction
 * (:120-227) evaluates the old traj_ while the solve runs, so every trajectory comes into force one solve late.  A setting of the batch, off by
 * default; with it off every entry is byte for byte what it is without this section.
 *
 * lat[batch][2] = {base, per_iteration}, seconds, finite and >= 0.  With a latency set the batch holds a second set of instance records, the
 * PUBLISHED trajectories, and srbm_control_tick[_dev] -- hence the ticks of srbm_controller_advance and srbm_gait_controller_advance -- read those.
 * Every other entry (srbm_get_trajectory, srbm_eval_trajectory, the step log, contact feedback, the updates) keeps working on the MPC's records.
 *
 * The rule.  The update that follows tick k (k > 0, k % ticks_per_update == 0) is update number u = k / ticks_per_update; it starts at
 *     t_start = (u * ticks_per_update) * tick_dt          an integer product, then one rounded product, as t_k everywhere
 * and for instance b, whose record holds qp_iters after that update (in a gait run: the installed winner's count), every rounded operation a
 * statement of its own,
 *     p   = per_iteration * qp_iters
 *     L   = base + p
 *     due = t_start + L
 * Before the targets kernel of tick j >= 1 let e = (j - 1) / ticks_per_update (integer division): the number of the last update started before
 * tick j, 0 for none.  Instance b is PENDING while the update number of its published record is below e.  A pending instance is published -- its
 * whole record copied from the MPC's set to the published set -- if
 *     due <= time[b]                                       time: the tick's own time array, t_j
 *  or the tick is forced: j % ticks_per_update == 0 and e >= 1.
 * The forced tick is the reference's thread structure: a solve cannot start before the last one was handed over, so the effective latency is
 * min(L, period); a forced publication with due > time[b] is counted as an overrun.  L = 0 everywhere is the behaviour without the setting (in
 * force from tick k + 1); base = ticks_per_update * tick_dt is the reference's thread, solves back to back, each in force one solve late;
 * per_iteration > 0 makes the latency follow the work of the solve, decided on the device without synchronisation.  The state is the published
 * update number of each instance and e follows from j: a rollout cut anywhere and continued is the same rollout.  (A rollout BEGUN at a later tick on
 * a state just set finds update number 0 in force and e > 0: its first ticks publish the trajectories found, the same bytes, as update e.)
 * What the setting is NOT: the MPC period stays batch-wide and fixed -- a latency beyond it is capped and counted, not turned into a slower MPC
 * rate; no model of the control tick's own computation time; no jitter.
 *
 * The latency record pub[batch][8]:
 *     0    update number in force (0: the trajectories found when the latency or the plant's state was set)
 *     1    publications
 *     2    overruns
 *     3    time of the last publication (-1: none)
 *     4    t_start of the trajectory in force (0 before the first publication)
 *     5    L of the last publication as computed
 *     6    max L over the publications
 *     7    sum of time - t_start over the publications, in publication order
 *
 * srbm_controller_set_latency: NULL removes the setting and frees the published set; otherwise allocates the set and fills it and the record from
 * the MPC's records as they are after the work queued so far.  Refused, naming the instance and the field, the batch untouched, for a value that is
 * not finite or negative.  srbm_wb_plant_set_state re-synchronises the published set with the MPC's and resets the record; srbm_batch_clone carries
 * the setting, the published set and the record.  An entry that replaces the MPC's trajectories from outside (srbm_set_warm_start_trajectory,
 * srbm_create_initial_run) does not touch the published set: set the latency, or the plant's state, after it.
 * srbm_controller_get_latency_record: pub[batch][8] after the work queued so far.  srbm_controller_get_published: srbm_get_trajectory on the
 * published set.  Both refused without a latency set.
 * srbm_controller_publish_dev: the publish kernel alone (csrc/srbm_mpc_latency.hiph) on the caller's time_dev[batch], for tests and host-driven
 * chains: update_number is e, t_start and force as above.  One launch on the batch's stream, no copy, no synchronisation; an instance that is not
 * published is not touched, record included.  Refused without a latency set, for update_number < 0, a t_start that is not finite, force not 0 / 1.
 *
 * In srbm_controller_advance and srbm_gait_controller_advance with a latency set the kernel runs before srbm_control_tick_dev of tick j, on the
 * tick's time array; contact feedback, the plant and the update are untouched (contact feedback edits the MPC's records, as
 * AdjustForCurrentContacts does in the reference's MPC thread).  The launch is skipped on the ticks on which the rule itself proves that no
 * instance is published: before the tick on which a solve of no iteration would be due, and after the tick on which the longest solve the solver
 * settings allow, or the forced tick, publishes -- with per_iteration = 0 that leaves the instance's one publication tick.  Before the FIRST tick of
 * every call (with e >= 1) the kernel is always launched: those ticks are computed for a rollout that has run since the update started, and in a
 * rollout begun at this tick on a state just set whatever the rule would have published earlier is due now; in a continued rollout that launch finds
 * nobody both pending and due.  Skipping changes no byte: the entry in one call, in one call per tick and the host-driven chain that launches
 * srbm_controller_publish_dev before every tick leave the same bytes, the latency record included, from tick 0 and from a later tick.
 * A tick can then read a trajectory up to two periods old: refused in addition, with both numbers in the message and nothing launched,
 * 2 * ticks_per_update * tick_dt >= num_nodes * dt.
 *
 * srbm_latency_publish_ticks_host needs no GPU: for a rollout from tick 0, lat[batch][2] and iters[batch][n_updates], iters[b][u - 1] the
 * iteration count of update u of instance b, publish_tick[batch][n_updates] <- the tick before whose targets kernel update u of instance b is
 * published and overrun[batch][n_updates] <- 1 if by force before it was due -- for the publications that fall among the ticks
 * first_tick .. first_tick + ticks - 1; -1 and 0 for the others.  The same rule functions as the kernel's. */
int srbm_controller_set_latency(srbm_batch* h, const double* lat);
int srbm_controller_get_latency_record(srbm_batch* h, double* pub);
int srbm_controller_get_published(srbm_batch* h, int first, int count, srbm_trajectory* out);
int srbm_controller_publish_dev(srbm_batch* h, const double* time_dev, int update_number, double t_start, int force);
int srbm_latency_publish_ticks_host(int batch, int first_tick, int ticks, int ticks_per_update, double tick_dt, const double* lat, const int* iters, int n_updates,
                                    int* publish_tick, int* overrun);

/* ---- sensor model: the control ticks of a rollout read a measurement of the plant's state, not the state ----
 * The reference's robot (hardware/hardware_robot.cpp) takes the base pose from motion capture at its own, slower rate (:484-485, :506), the base
 * linear velocity from a finite difference of the two newest samples (:507), the angular velocity from the gyro (:519-521), passes base and joint
 * velocities through a first-order low-pass filter (:152-174, LPF at :676-679), and everything carries noise.  A setting of the batch, off by default;
 * with it off every entry is byte for byte what it is without this section.  With it set, every control tick of srbm_controller_advance and
 * srbm_gait_controller_advance reads a MEASURED (qm, vm) that one kernel (srbm_k_measure, csrc/srbm_sensors.hiph) makes from the plant's true (q, v)
 * just before the tick -- and so do ReconstructState, the targets, the whole-body QP and the state / ee handed to the MPC update or the gait step.
 * The plant, the push, the ground's contact state and contact feedback (the ground's cs: foot-force sensing is out of scope), the latency rule and
 * the tick-log head (fields 0..46 and 51..56) keep working on the true state.
 *
 * sens[batch][16] and seed[batch] (64 bits, any value) per instance:
 *     0        mocap_ticks, integer 1..64: the base pose is sampled on ticks k with k % mocap_ticks == 0 and held in between
 *     1        mocap_delay, integer 0..3: the tick reads the sample taken that many samples before the newest
 *     2, 3     sigma_p (m, per axis), sigma_r (rad, per axis) of a pose sample
 *     4        base linear velocity source.  0: the plant's v[0..3).  1: the finite difference of the two newest available samples
 *     5        sigma_v (m/s) of the linear velocity (source 0; source 1 inherits the pose noise)
 *     6, 7..9  gyro sigma_w, gyro bias[3]
 *     10, 11   sigma_qj, sigma_vj of the twelve joint angles / rates
 *     12, 13   low-pass x of the six base velocities and of the joint rates, 0: no filter; x = tan(pi fpass / fsample) in the reference
 *     14, 15   0
 * Refused, naming instance and field, the batch untouched: a value that is not finite; a negative sigma or x; a count that is no integer or out of
 * range; a source other than 0 / 1; entries 14, 15 not 0.
 *
 * Noise.  Counter-based, so a rollout cut anywhere is the same rollout: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants
 * 0x9E3779B9, 0xBB67AE85), key (low, high word of the instance's seed), counter (tick k, channel c, 0, 0).  The four output words are summed exactly
 * in 64 bits, s converts to double exactly, and z = (s 2^-32 - 2) * 1.7320508075688772: zero mean, unit variance, |z| <= 2 sqrt(3), the same bits
 * on host and device.  Channels: 0..2 position, 3..5 orientation, 6..8 linear velocity, 9..11 gyro, 12..23 joint angles, 24..35 joint rates.
 * A channel whose sigma is 0 copies its input -- no arithmetic on it at all -- and so does a gyro axis whose bias is 0.
 * Every rounded operation below is one IEEE operation, in the order written.
 * Pose.  On a sample tick: position p + sigma_p z; orientation q (x) (delta / 2, 1), delta = sigma_r z, the terms of each component in the order of
 *     x = a3 b0 + a0 b3 + a1 b2 - a2 b1,  y = a3 b1 - a0 b2 + a1 b3 + a2 b0,  z = a3 b2 + a0 b1 - a1 b0 + a2 b3,  w = a3 b3 - a0 b0 - a1 b1 - a2 b2
 * (xyzw, a = q, b3 = 1) summed left to right, then scaled by (3 - |.|^2) / 2, the squares summed x, y, z, w; skipped altogether at sigma_r == 0.
 * The sample goes into slot n % 5 of a ring of 5, n the samples taken before.  The tick's base pose is the ring entry mocap_delay behind the newest.
 * The ring is pre-filled with the true initial pose, so early ticks read that.
 * Linear velocity, source 1: (p_avail - p_prev) / (mocap_ticks * tick_dt), the ring entries at and one behind the available one, each component
 * divided, then rotated into the frame of the plant's v[0..3) -- the body frame -- by the transpose of the available sample's rotation matrix
 * (R = Eigen's Quaterniond::matrix(); component i is R0i w0 + R1i w1 + R2i w2 left to right, Rii = 1 - 2 (. + .), Rij = 2 (. +- .)).  It is zero
 * while the two entries are the pre-fill.
 * Gyro: omega + bias + sigma_w z.  Joints: q_j + sigma_qj z, v_j + sigma_vj z.
 * Filter, once per tick and velocity component: out = (x (cur + prev) + (1 - x) prev_out) / (x + 1), formed as a (cur + prev) + c prev_out with
 * a = x / (1 + x), c = (1 - x) / (1 + x) computed once on the host; prev and prev_out start at the true initial v; x == 0: out = cur.
 * The transparent model -- count 1, delay 0, source 0, no sigma, no bias, no filter -- makes (qm, vm) the bytes of (q, v).
 *
 * Sensor state ms[batch][72], carried from tick to tick in the batch:
 *     0            pose samples taken
 *     1 + 7 s + i  component i of ring slot s = 0..4: position [3], quaternion xyzw [4]
 *     36 + j       the filter's prev of velocity component j = 0..17 (the unfiltered measurement of the last tick)
 *     54 + j       the filter's prev_out (the measurement of the last tick)
 * Sensor record srec[batch][8] since the state was set:
 *     0, 1         ticks measured, pose samples taken
 *     2..7         running maxima of |pm - p|_inf, 1 - (qm . q)^2 (0 where qm equals q component for component), |vm_lin - v_lin|_inf,
 *                  |wm - w|_inf, |qm_j - q_j|_inf, |vm_j - v_j|_inf
 *
 * srbm_controller_set_sensors: NULL sens removes the setting and frees its buffers; otherwise stores the setting and starts the sensor state, the
 * record (zero) and the last measurement from the plant's state as it is after the work queued so far (without a plant state: at
 * srbm_wb_plant_set_state).  srbm_wb_plant_set_state re-initialises state and record from the state being set; srbm_batch_clone carries setting,
 * state, record and last measurement.  srbm_controller_get_sensors: the setting back.  _get_sensor_state / _set_sensor_state: ms[batch][72]
 * (set: the sample count must be an integer 0 .. 2^52).  _get_sensor_record: srec[batch][8].  _get_measured: the last (qm[batch][19], vm[batch][18]);
 * either may be NULL.  All refused without the setting.
 * srbm_controller_measure_dev: the kernel alone on the caller's true q_dev[batch][19], v_dev[batch][18] and output arrays (which must not be the
 * inputs), for tests and host-driven chains: it advances the batch's sensor state and record by tick `tick`.  One launch on the batch's stream, no
 * copy, no synchronisation.  Refused without the setting, before a plant state was set, for tick < 0 or a tick_dt that is not finite and > 0.
 * In srbm_controller_advance the kernel runs directly before srbm_control_tick_dev of tick k (after a latency publication, if any) and the tick
 * gets the batch's (qm, vm) in the place of the plant's arrays; nothing else in the loop changes.
 * What it is NOT: no foot-force or contact sensing (contact feedback keeps reading the ground); no accelerometer; no state estimator beyond the
 * reference's differencing and filtering; no dropped packets; the reference's substitution for a packet that was not updated (:142-144) is not
 * modelled.
 *
 * Three entries need no GPU.  srbm_sensor_philox_host: one Philox4x32-10 block, words as bit patterns.  srbm_sensor_state_init_host:
 * ms[batch][72] of plants at q[batch][19], v[batch][18].  srbm_sensor_measure_host: the same model function the kernel compiles, over a recorded
 * sequence q_true[ticks][batch][19], v_true[ticks][batch][18] for ticks first_tick .. first_tick + ticks - 1: ms_inout and srec_inout move,
 * qm_out[ticks][batch][19] and vm_out[ticks][batch][18] are written.  Refused as srbm_controller_set_sensors refuses. */
#define SRBM_SENSOR_DOUBLES 16
#define SRBM_SENSOR_STATE_DOUBLES 72
#define SRBM_SENSOR_RECORD_DOUBLES 8
int srbm_controller_set_sensors(srbm_batch* h, const double* sens, const long long* seed);
int srbm_controller_get_sensors(srbm_batch* h, double* sens, long long* seed);
int srbm_controller_get_sensor_state(srbm_batch* h, double* ms);
int srbm_controller_set_sensor_state(srbm_batch* h, const double* ms);
int srbm_controller_get_sensor_record(srbm_batch* h, double* srec);
int srbm_controller_get_measured(srbm_batch* h, double* q, double* v);
int srbm_controller_measure_dev(srbm_batch* h, int tick, double tick_dt, const double* q_dev, const double* v_dev, double* qm_dev, double* vm_dev);
int srbm_sensor_philox_host(const int* counter4, const int* key2, int* out4);
int srbm_sensor_state_init_host(int batch, const double* q, const double* v, double* ms);
int srbm_sensor_measure_host(int batch, int first_tick, int ticks, double tick_dt, const double* sens, const long long* seed, const double* q_true,
                             const double* v_true, double* ms_inout, double* srec_inout, double* qm_out, double* vm_out);

/* ---- results (all copied to host) ---- */
/* sizes[batch][8] = n, m, n_eq, n_ineq, n_force_vars, n_pos_vars, n_td_rows, n_force_samples */
int srbm_get_sizes(srbm_batch* h, int* sizes);
/* status[batch] = mpc::SolveQuality (mpc/include/qp/qp_interface.h:12-22); err[batch] = error bits (0 = none).
 * Both describe the LAST solve only.  Error bits (conditions on which the reference throws, plus two of this library): 1 time before the first knot,
 * 2 time beyond the last knot, 4 invalid time, 8 force node not mutable, 16 beyond the capacity of the build (status Other), 32 RemovePoly on an empty
 * spline, 64 touch-down index, 128 a pivot of the normal matrix was regularised, 256 internal invariant violated (a dense state row with a non-zero
 * outside the force variables of its coordinate: never observed; the compact storage of those rows rests on it), 512 a bounded wait of the step
 * queue ran out (multi-step launches of a batch larger than the chip hand out (instance, step) items to a resident grid; never observed).
 *
 * Refused solves and the gait step.  A schedule that needs more spline variables, force samples or knots per foot than the build holds
 * (srbm_get_capacity) is REFUSED by the assembly: status 8 (Other), bit 16, one solve counted as not solved.  No QP was assembled: the instance's
 * trajectory (node states, knot tables, init_time) and its last solution stay those of its last accepted solve, while srbm_get_sizes reports the
 * sizes of the schedule that did not fit.  Until the instance's next solve:
 *   - condensing, the interior-point solve and the update return at once, in the one-step and in the multi-step launches (every later step
 *     of a multi-step launch assembles again -- and is refused again while the schedule stays);
 *   - srbm_gait_compute_sensitivity leaves the instance's sensitivity workspace as it was (only its LU-failure flag is set) and
 *     srbm_gait_get_sensitivity returns a zero row for it; srbm_gait_compute_gradient writes a zero gradient row and valid = 0; the instance is
 *     never "ready" in the advance entries, whatever srbm_gait_set_gradient supplied: a line-search run gives it the plain update (refused again,
 *     imin = -1).  Bit 16 raised by the gait step itself (more than 32 contact times per instance, more than 16 per foot) has the same effect;
 *   - srbm_gait_line_search has no ready mask: the instance's ten candidates solve x_k + (i/10) step like any other's -- those that do not fit
 *     are refused one by one (srbm_gait_get_candidate_status), one that fits may win;
 *   - srbm_export_qp and srbm_gait_get_param_partials fail ("... was refused for capacity ...") and write nothing;
 *   - every other read-back entry, the step-log and tick kernels and srbm_pack_results bound their loops by the capacities of the build, not by
 *     the sizes of the instance, and show the last accepted solve. */
int srbm_get_status(srbm_batch* h, int* status, int* err);
/* Sticky accumulators over every solve since creation / the last clear (multi-step launches overwrite status and err each
 * step; the step log, srbm_step_log_*, keeps both per step): acc[batch][4] = {all error bits raised, solves, solves not in {Solved, SolvedInacc},
 * of those MaxIter} */
int srbm_get_status_accumulated(srbm_batch* h, int* acc);
int srbm_clear_status_accumulators(srbm_batch* h);
/* counters over the same span: c[4] = {solves, solves ended by the step rule, lower-start attempts, attempts repeated from the standard start} */
int srbm_get_solver_counters(srbm_batch* h, long long* c4);
/* stats[batch][8] = alpha, cost (GetCost), L1 dynamics defect, step norm, qp iterations, res_primal, res_dual, gap_rel */
int srbm_get_stats(srbm_batch* h, double* stats);
/* objective of the QP at its raw minimiser, cost[batch] (the "QP Cost" column of MPC::PrintStatLineToFile, mpc/mpc.cpp:974-989) */
int srbm_get_qp_cost(srbm_batch* h, double* cost);
/* MPC::GetQPSolution (prev_qp_sol after the line search), x[batch][ld]; ld >= n_max */
int srbm_get_qp_solution(srbm_batch* h, double* x, int ld);
int srbm_get_raw_qp_minimiser(srbm_batch* h, double* x, int ld);
/* ClarabelInterface::GetDualSolution in the reference's row order; z[batch][ld] */
int srbm_get_dual_solution(srbm_batch* h, double* z, double* s, int ld);
/* Trajectory::GetStates, states[batch][N+1][13] */
int srbm_get_trajectory_states(srbm_batch* h, double* states);
/* knot tables of one instance: times[4][32], kinds[4][32] (0 LO, 1 TD, 2 stance-interior, 3 mid-swing), nk[4],
 * fvals[4][3][32][2], pvals[4][2][32], box[2] */
int srbm_get_knots(srbm_batch* h, int inst, double* times, int* kinds, int* nk, double* fvals, double* pvals, double* box);
/* Dense expansion of the structured QP of the LAST solve of one instance into the reference's layout
 * (rows/cols as SURVEY.md Appendix A): A[m][n], b[m], P[n][n], q[n].  Debug / parity-test aid. */
int srbm_export_qp(srbm_batch* h, int inst, double* A, double* b, double* P, double* q);
/* What the condensing left in the work record of one instance at its LAST solve, at the capacities of the loaded build (srbm_get_capacity: N_max,
 * n_u_max): H[n_u_max (n_u_max + 1) / 2] packed lower by rows, g[n_u_max], the compact dense state rows Sig[2 (N_max - 3)][n_u_max] (row 2 (k - 4) + c
 * = position c of node k on the force variables of coordinate c over the four feet), sig0[2 (N_max - 3)], the instance's n_u and its error bits.
 * Debug / parity-test aid like srbm_export_qp. */
int srbm_debug_get_condensed(srbm_batch* h, int inst, double* H, double* g, double* Sig, double* sig0, int* nu, int* err);
/* result records for collection across GPUs (one RCCL all-gather in bench.py): out_dev[batch][ld] on
 * the handle's stream.  Layout of one record (doubles), NX = 12 (N+1) + n_u_max, NM = 12 (N+1) + 6 * samples_max + 16 (N-3) + 16 with the capacities of the loaded build
 * (srbm_get_capacity: 160 / 120 in the standard build, 240 / 200 in the LARGE one):
 *   [0..8)  status, n, m, cost, alpha, err (sticky bits since the last clear), qp_iters, init_time
 *   [8 .. 8+NX)           x[0..n)   primal (prev_qp_sol), zero padded
 *   [8+NX .. 8+NX+NM)     z[0..m)   dual vector in the reference's row order, zero padded
 *   [8+NX+NM .. +36)      contact-time counts of the 4 feet, then 4 x 8 contact times
 * srbm_result_record_doubles(N) = 8 + NX + NM + 36.  A shorter ld truncates the record (ld >= 8). */
int srbm_result_record_doubles(int num_nodes);
int srbm_pack_results_dev(srbm_batch* h, double* out_dev, int ld);
/* the same records into a HOST buffer out[batch][ld] (synchronous) */
int srbm_pack_results(srbm_batch* h, double* out, int ld);

/* ---- multi-GPU: collecting the solved trajectories of all shards (north_star: "partitioned across the 8 GPUs of one node with an RCCL all-gather
 * over xGMI only to collect solved trajectories"; the reference's only batch is the 10-thread line search, mpc/gait_optimizer.cpp:688-721; the host
 * that would call this is the MPC thread of controllers/mpc_controller.cpp:286-399, one per GPU) ----
 * One process per GPU, each owning a batch of the SAME size (contiguous shards of the global batch).  srbm_allgather_results packs this rank's
 * result records (srbm_pack_results_dev layout, ld = srbm_result_record_doubles(N)) straight into its slot of out_dev and runs ONE in-place
 * ncclAllGather (RCCL) on the batch's stream: out_dev[world * batch][ld] on every rank, rank r's records at rows [r * batch, (r + 1) * batch).
 * Asynchronous like every *_dev entry: srbm_synchronize (or work queued behind it on srbm_get_stream) before out_dev is read.
 * `comm` is a plain ncclComm_t of <rccl/rccl.h> -- the caller's own (ncclCommInitRank on its side), or one made by the helpers below for hosts
 * that do not link RCCL themselves (ctypes, bench.py).  The library does not link RCCL: it binds the copy already loaded in the process
 * (librccl.so / librccl.so.1), else loads librccl.so.1, at the first of these calls; SRBM_RCCL_LIB overrides the name.  No RCCL, no call: they fail loudly. */
struct ncclComm;
typedef struct ncclComm* ncclComm_t;               /* identical to the typedef in <rccl/rccl.h> */
#define SRBM_RCCL_UNIQUE_ID_BYTES 128              /* sizeof(ncclUniqueId) */
int srbm_allgather_results(srbm_batch* h, ncclComm_t comm, double* out_dev);
/* the same for the rollout summaries (see "rollout summaries" above): out_dev[world * batch][SRBM_ROLLOUT_SUMMARY_DOUBLES] */
int srbm_rollout_allgather_dev(srbm_batch* h, ncclComm_t comm, double* out_dev);
/* ... and for the tick summaries (see "tick summaries" above): out_dev[world * batch][SRBM_TICK_SUMMARY_DOUBLES] */
int srbm_tick_summary_allgather_dev(srbm_batch* h, ncclComm_t comm, double* out_dev);
/* ncclGetUniqueId on one rank (bytes travel to the others by whatever the host uses for its rendezvous), ncclCommInitRank on the batch's device, ncclCommDestroy */
int srbm_rccl_get_unique_id(void* id_bytes);
int srbm_rccl_comm_init_rank(srbm_batch* h, int world, int rank, const void* id_bytes, ncclComm_t* comm_out);
int srbm_rccl_comm_destroy(ncclComm_t comm);
/* measurement aids: HIP-event timing of the dominant kernel (srbm_k3_ipm) on the launch stream, and running totals
 * of executed IPM iterations / algorithmic flops (SURVEY.md section 8d formula) summed over the batch */
int srbm_enable_kernel_timing(srbm_batch* h, int max_launches);
int srbm_get_kernel_timing(srbm_batch* h, double* total_ms, int* launches);
/* ... and launch by launch: ms_each[min(launches, max_launches)] in launch order (bench.py prices the MEDIAN region with its own launch) */
int srbm_get_kernel_timings(srbm_batch* h, double* ms_each, int max_launches, int* launches);
int srbm_get_work_counters(srbm_batch* h, double* total_ipm_iterations, double* total_algorithmic_flops);
/* matrix-core instructions (v_mfma_f64_16x16x4_f64, 2048 flop each, counted per wave) EXECUTED by the condensing and IPM
 * phases, summed over the batch: the executed-flop side of the roofline (the algorithmic figure counts a dense SYRK that the
 * structured assembly never performs) */
int srbm_get_executed_mfma(srbm_batch* h, double* total_mfma_instructions);
/* bytes of HBM held per instance (persistent record + per-solve workspace) */
long srbm_bytes_per_instance(void);

#ifdef __cplusplus
}
#endif
#endif
