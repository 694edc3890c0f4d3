// Host side of the batched SRBM RTI path: the C-ABI of include/srbm_rti.h over the HIP kernels.
// Mirrors the call sequence of mpc::MPC / mpc::MPCSingleRigidBody (reference file:line cited in the header).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: RCCL is bound at run time (srbm_allgather_results), the library does not link it
#include <dlfcn.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "srbm_k4_update.hiph"
#include "srbm_gait.hiph"
#include "srbm_plant.hiph"
#include "srbm_fused.hiph"
#include "srbm_gait_rollout.hiph"
#include "srbm_ik.hiph"
#include "srbm_wbc.hiph"
#include "srbm_tick.hiph"
#include "srbm_wb_plant.hiph"
#include "srbm_wb_fd.hiph"
#include "srbm_wb_ground.hiph"
#include "srbm_wb_terrain.hiph"
#include "srbm_wb_joints.hiph"
#include "srbm_wb_wrench.hiph"
#include "srbm_command.hiph"
#include "srbm_contact_feedback.hiph"
#include "srbm_mpc_latency.hiph"
#include "srbm_sensors.hiph"
#include "srbm_rollout_summary.hiph"
#include "srbm_tick_summary.hiph"
#include "srbm_batch.hiph"
#include "srbm_dense_hooks.hiph"
#include "../../include/srbm_rti.h"

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return -1; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// temporaries of the debug / export entries: released on every return path
struct DevTemps {
    std::vector<void*> ptrs;
    ~DevTemps() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t alloc(T** out, size_t bytes) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T*>(p);
        return e;
    }
};

// The fields of SrbmParams that belong to ONE instance: its constructor data (srbm_batch_create_each) and its costs (the cost setters).  Every other
// field of a record is batch-wide: the same in all records, taken from srbm_batch::hp.
struct InstModel {
    double mu_fric, force_bound, force_cost, box0[2];
    double mass, Ir[9], Ir_inv[9];
    double Q[144], w[12], Phi[144], Phi_w[12];
};

struct srbm_batch {
    int batch = 0, device = 0;
    SrbmParams hp{};                 // host copy of the batch-wide parameters (its per-instance fields are not used: see im)
    std::vector<InstModel> im;       // per-instance parameters [batch]
    double hip_xy[8] = {};           // srbm_model::hip_xy as given at creation (hp.hip holds GetCOMToHip of it)
    std::vector<SrbmParams> recs;    // host image of dp: hp with instance b's fields laid over it, one record per instance
    SrbmParams* dp = nullptr;        // [batch] on the device: every kernel reads the record of the instance it works on
    unsigned params_gen = 0;         // counts the changes of hp / im (the gait's candidate batch re-derives its records when it moves)
    SrbmInst* insts = nullptr;
    SrbmWork* works = nullptr;
    double *d_state = nullptr, *d_time = nullptr, *d_ee = nullptr;
    double *d_plant = nullptr, *d_push = nullptr;   // closed-loop harness (srbm_plant.hiph): states [batch][13], pushes [batch][SRBM_PUSH_DOUBLES] {time, impulse[6]}
    bool push_set = false;
    double* d_dt = nullptr;          // the node step dt [batch]: the `period` of every launch that has no other (SrbmPlantArgs)
    double* d_period = nullptr;      // MPC period of the closed-loop protocols [batch] (srbm_plant_set_period), allocated at the first set
    std::vector<double> period;      // its host copy; empty: none set, every instance runs at the node step dt
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    int n_cu = 0;
    SrbmQueue* queues = nullptr;     // step queues of multi-step launches of a batch larger than the chip (srbm_fused.hiph), allocated at first use
    bool queued_ok = true;           // SRBM_NO_STEP_QUEUE=1 in the environment: such launches as one workgroup per instance (A/B, tests)
    int last_launch_kernel = 0;      // kernel of the last srbm_rti_advance / srbm_closed_loop_advance with steps > 0 (srbm_debug_get_launch_info)
    int last_launch_steps = 0;
    bool params_dirty = true;
    // optional HIP-event timing of the dominant kernel (srbm_k3_ipm) on the launch stream
    bool timing = false;
    std::vector<hipEvent_t> ev_start, ev_stop;
    std::vector<int> ev_steps;        // RTI steps covered by each timed launch (1 for the stand-alone IPM kernel)
    size_t ev_used = 0;
    int gait_refs = 0;               // live srbm_gait handles borrowing this batch (and its stream)
    double last_tol_step = 0.0;      // tol_step of the last solve launched on this batch: > 0 means its duals may not be at the gap tolerance
    SrbmWbcParams* d_wbc = nullptr;  // whole-body QP model and gains (row f3), set by srbm_set_wbc_model
    void* d_scratch = nullptr;       // staging buffer of the small host->device entry points (grown on demand, never per call)
    size_t scratch_bytes = 0;
    void* h_stage = nullptr;         // pinned host mirror of d_scratch for the per-tick entries: ONE copy in, ONE copy out per call
    size_t stage_bytes = 0;
    double* d_log = nullptr;         // step log [log_cap][batch][SRBM_STEP_LOG_DOUBLES] (srbm_steplog.hiph), nullptr: logging off
    int log_cap = 0, log_used = 0;   // slots allocated; the cursor: slots written by the launches queued so far
    // rollout summaries (srbm_rollout_summary.hiph): the log folded per instance, nullptr: off
    double* d_sum = nullptr;         // [batch][SRBM_ROLLOUT_SUMMARY_DOUBLES]
    double* d_sum_ref = nullptr;     // the references [batch][SRBM_ROLLOUT_REF_DOUBLES]
    SrbmRolloutCriteria sum_crit{};  // the criteria, a kernel argument
    std::vector<double> sum_init;    // host image of the summaries after a reset (the source of the asynchronous copy that resets them)
    // control tick (srbm_control_tick, srbm_tick.hiph): MPCController's member state for the batch, allocated by srbm_control_tick_reset
    double* d_tick_q = nullptr;              // q_des_ [batch][19]
    SrbmTickRec* d_tick_rec = nullptr;       // the targets of the tick under way [batch], between its two kernels
    // whole-controller rollouts (srbm_controller_advance, srbm_wb_plant.hiph), allocated by srbm_wb_plant_set_state: the plant's (q, v), the times of
    // two ticks in turn and the outputs of the tick under way (WbBuf lays them out)
    double* d_wb = nullptr;          // [WB_DOUBLES][batch]
    int* d_wb_int = nullptr;         // [WB_INTS][batch]
    double* d_tlog = nullptr;        // tick log [tlog_cap][batch][SRBM_TICK_LOG_DOUBLES], nullptr: logging off
    int tlog_cap = 0, tlog_used = 0; // slots allocated; the cursor
    // tick summaries (srbm_tick_summary.hiph): the tick log folded per instance, nullptr: off
    double* d_tsum = nullptr;        // [batch][SRBM_TICK_SUMMARY_DOUBLES]
    double* d_tsum_ref = nullptr;    // the references [batch][SRBM_TICK_REF_DOUBLES]
    SrbmTickCriteria tsum_crit{};    // the criteria, a kernel argument
    std::vector<double> tsum_init;   // host image of the summaries after a reset
    // the torque-driven plant (srbm_wb_fd.hiph): the kind srbm_controller_advance launches, the actuators and the plant's own bodies
    int fd_kind = 0;                 // 0: the QP-acceleration plant, 1: the torque-driven plant (srbm_wb_plant_set_kind)
    int fd_substeps = 1;
    double* d_fd_act = nullptr;      // [batch][WBFD_ACT_DOUBLES] kp, kd, torque limit; nullptr: not set (srbm_wb_plant_set_actuators)
    SrbmBody* d_fd_bodies = nullptr; // [batch][13]; nullptr: the controller's bodies (srbm_wb_plant_set_bodies_each)
    // the ground of the torque-driven plant (srbm_wb_ground.hiph)
    double* d_ground = nullptr;      // [batch][WBG_GROUND_DOUBLES]; nullptr: no ground, kind 1 holds the planned feet (srbm_wb_plant_set_ground)
    double* d_cs = nullptr;          // the contact state [batch][WBG_CS_DOUBLES], allocated with d_wb
    // the terrain of that ground (srbm_wb_terrain.hiph)
    double* d_terrain = nullptr;     // [batch][WBG_TERRAIN_PATCHES][WBT_PATCH_DOUBLES]; nullptr: the ground is its plane (srbm_wb_plant_set_terrain)
    int terrain_patches = 0;         // the n_patches of the call that set it: what in_contact may hold
    // contact feedback of the rollout's MPC update (srbm_contact_feedback.hiph)
    int contact_fb = 0;              // 1: the update ticks of srbm_controller_advance run the feedback kernel (srbm_controller_set_contact_feedback)
    double* d_fb = nullptr;          // the feedback record [batch][SRBM_FB_DOUBLES], allocated with d_wb
    // MPC computation latency of the rollout (srbm_mpc_latency.hiph, srbm_controller_set_latency)
    SrbmInst* pub_insts = nullptr;   // the published trajectories [batch], what the control tick reads; nullptr: no latency set, it reads insts
    double* d_lat = nullptr;         // lat[batch][SRBM_LAT_DOUBLES], allocated with pub_insts
    double* d_pub = nullptr;         // the latency record [batch][SRBM_PUB_DOUBLES], allocated with pub_insts
    std::vector<double> lat;         // host copy of d_lat (the launches srbm_controller_advance may skip follow from it)
    std::vector<double> pub_init;    // host image of the record after a reset (the source of the asynchronous copy that resets it)
    // sensor model of the rollout (srbm_sensors.hiph, srbm_controller_set_sensors): one allocation d_sens, nullptr: no sensors set, the ticks read the plant
    double* d_sens = nullptr;        // [batch] x {record SRBM_SENS_DEV_DOUBLES, state, record of the run, qm[19], vm[18]}: sens_buf(); then seed[batch]
    bool sens_ready = false;         // the sensor state was initialised from a plant state
    std::vector<double> sens;        // host copy of the caller's sens[batch][SRBM_SENS_DOUBLES]
    std::vector<unsigned long long> sens_seed;
    // the joint model of the torque-driven plant (srbm_wb_joints.hiph, srbm_wb_plant_set_joints): one allocation, nullptr: no joint model set
    double* d_joints = nullptr;      // joints[batch][12][8], stops[batch][2], js[batch][12], jrec[batch][8]: joint_buf()
    std::vector<double> joints;      // host copy of the caller's joints, then stops
    // the wrench schedule of the torque-driven plant (srbm_wb_wrench.hiph, srbm_wb_plant_set_wrenches): one allocation, nullptr: no schedule set
    double* d_wrench = nullptr;      // wrenches[batch][8][16] (padded with empty slots), wrec[batch][8]: wrench_buf()
    std::vector<double> wrenches;    // host copy of the caller's wrenches[batch][wrench_events][16]
    int wrench_events = 0;
    // the command schedule of the rollout (srbm_command.hiph, srbm_controller_set_commands): one allocation, nullptr: no schedule set
    double* d_cmd = nullptr;         // cmds[batch][cmd_events][28], cstate[batch][4], crec[batch][32]: cmd_buf()
    std::vector<double> cmds;        // host copy of the caller's cmds
    std::vector<double> cmd_init;    // host image of state and record after a reset (the source of the asynchronous copy that resets them)
    int cmd_events = 0;
};
static int batch_scratch(srbm_batch* h, size_t bytes, void** out) {
    if (bytes > h->scratch_bytes) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_scratch) HIPCHK(hipFree(h->d_scratch));
        h->d_scratch = nullptr; h->scratch_bytes = 0;
        HIPCHK(hipMalloc(&h->d_scratch, bytes));
        h->scratch_bytes = bytes;
    }
    *out = h->d_scratch;
    return 0;
}
// device scratch + a pinned host buffer of the same size and layout
static int batch_stage(srbm_batch* h, size_t bytes, void** dev, void** host) {
    if (batch_scratch(h, bytes, dev)) return -1;
    if (bytes > h->stage_bytes) {
        if (h->h_stage) HIPCHK(hipHostFree(h->h_stage));
        h->h_stage = nullptr; h->stage_bytes = 0;
        HIPCHK(hipHostMalloc(&h->h_stage, bytes, hipHostMallocDefault));
        h->stage_bytes = bytes;
    }
    *host = h->h_stage;
    return 0;
}
// The layout of a staging buffer: sub-buffers handed out in order, each at an 8-byte boundary, at the same offset in the device scratch and in
// its pinned host mirror.  add() lays the parts out, stage() / scratch() take the buffer (batch_stage / batch_scratch), dev() / host() place them.
template <class T> struct Part { size_t off, n; size_t bytes() const { return sizeof(T) * n; } };
struct Carve {
    size_t end = 0;
    char *d = nullptr, *hm = nullptr;
    template <class T> Part<T> add(size_t n) { const size_t off = (end + 7) / 8 * 8; end = off + sizeof(T) * n; return {off, n}; }
    int stage(srbm_batch* h) { void *dv, *hv; if (batch_stage(h, end, &dv, &hv)) return -1; d = static_cast<char*>(dv); hm = static_cast<char*>(hv); return 0; }
    int scratch(srbm_batch* h) { void* dv; if (batch_scratch(h, end, &dv)) return -1; d = static_cast<char*>(dv); return 0; }
    template <class T> T* dev(Part<T> p) const { return reinterpret_cast<T*>(d + p.off); }
    template <class T> T* host(Part<T> p) const { return reinterpret_cast<T*>(hm + p.off); }
    template <class A, class B> static size_t span(Part<A> first, Part<B> last) { return last.off + last.bytes() - first.off; }   // bytes first..last
};

// ---------------- host helpers ----------------
struct Copy { void* dst; const void* src; size_t bytes; };        // one hipMemcpy; dst == nullptr: an optional output that was not asked for
static int copy_each(std::initializer_list<Copy> cs, hipMemcpyKind kind) {
    for (const Copy& c : cs) if (c.dst) HIPCHK(hipMemcpy(c.dst, c.src, c.bytes, kind));
    return 0;
}
// device -> host copies, after the work queued on the batch's stream
static int fetch(srbm_batch* h, std::initializer_list<Copy> cs) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return copy_each(cs, hipMemcpyDeviceToHost);
}
// the field at `offset` of instance `inst`'s SrbmWork (device address)
static const void* work_field(const srbm_batch* h, int inst, size_t offset) { return reinterpret_cast<const char*>(h->works + inst) + offset; }
// one SrbmWork field of every instance, `count` doubles of it per row of `out`
static int fetch_work_field(srbm_batch* h, size_t offset, size_t count, double* out, int ld) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((size_t)ld < count) return fail("leading dimension too small");
    HIPCHK(hipMemcpy2D(out, sizeof(double) * ld, reinterpret_cast<const char*>(h->works) + offset, sizeof(SrbmWork), sizeof(double) * count,
                       h->batch, hipMemcpyDeviceToHost));
    return 0;
}
// the SrbmInst array on the host, after the work queued on the batch's stream: f(b, instance b) for every instance
template <class F> static int each_inst(srbm_batch* h, F f) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<SrbmInst> v(h->batch);
    HIPCHK(hipMemcpy(v.data(), h->insts, sizeof(SrbmInst) * (size_t)h->batch, hipMemcpyDeviceToHost));
    for (int b = 0; b < h->batch; b++) f(b, v[b]);
    return 0;
}
// the record of instance b: the batch-wide fields, then the instance's own
static SrbmParams inst_params(const srbm_batch* h, int b) {
    SrbmParams p = h->hp;
    const InstModel& m = h->im[b];
    p.mu_fric = m.mu_fric; p.force_bound = m.force_bound; p.force_cost = m.force_cost;
    p.box0[0] = m.box0[0]; p.box0[1] = m.box0[1];
    p.mass = m.mass;
    std::memcpy(p.Ir, m.Ir, sizeof(p.Ir)); std::memcpy(p.Ir_inv, m.Ir_inv, sizeof(p.Ir_inv));
    std::memcpy(p.Q, m.Q, sizeof(p.Q)); std::memcpy(p.w, m.w, sizeof(p.w));
    std::memcpy(p.Phi, m.Phi, sizeof(p.Phi)); std::memcpy(p.Phi_w, m.Phi_w, sizeof(p.Phi_w));
    // per instance: a full Q on one instance sends that instance alone down the 12x12 path of the condensing kernel
    p.q_diag = 1;
    for (int i = 0; i < 144; i++) if (i % 13 != 0 && (p.Q[i] != 0.0 || p.Phi[i] != 0.0)) p.q_diag = 0;
    return p;
}
// hp or im changed: the records go to the device before the next launch
static void params_changed(srbm_batch* h) { h->params_dirty = true; h->params_gen++; }
static int upload_params(srbm_batch* h) {
    if (!h->params_dirty) return 0;
    h->recs.resize(h->batch);
    for (int b = 0; b < h->batch; b++) h->recs[b] = inst_params(h, b);
    HIPCHK(hipMemcpyAsync(h->dp, h->recs.data(), sizeof(SrbmParams) * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    h->params_dirty = false;
    return 0;
}
static void inv3(const double* m, double* r) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], hh = m[7], i = m[8];
    const double det = a * (e * i - f * hh) - b * (d * i - f * g) + c * (d * hh - e * g);
    r[0] = (e * i - f * hh) / det; r[1] = (c * hh - b * i) / det; r[2] = (b * f - c * e) / det;
    r[3] = (f * g - d * i) / det; r[4] = (a * i - c * g) / det; r[5] = (c * d - a * f) / det;
    r[6] = (d * hh - e * g) / det; r[7] = (b * g - a * hh) / det; r[8] = (a * e - b * d) / det;
}
// the batch's device made current, its parameters uploaded if they changed: the start of every entry that launches
static int use_batch(srbm_batch* h) {
    HIPCHK(hipSetDevice(h->device));
    return upload_params(h);
}
// the IPM variant of every launch path: the _long kernels beyond K3_SHORT_N nodes (srbm_k3_ipm.hiph)
static bool k3_long(const srbm_batch* h) { return h->hp.N > K3_SHORT_N; }
// The eight multi-step kernels (srbm_fused.hiph) by [step queues][_long][_logged]: alloc_batch raises the dynamic-LDS limit of each, launch_fused
// launches one.  Their argument lists share the first nine; the queued ones go on with (queues, batch), the logged ones end with the log arguments.
static const void* multi_step_kernel(bool queued, bool long_n, bool logged) {
#define K(name) reinterpret_cast<const void*>(name)
    static const void* const table[2][2][2] = {{{K(srbm_rti_fused), K(srbm_rti_fused_logged)}, {K(srbm_rti_fused_long), K(srbm_rti_fused_long_logged)}},
                                               {{K(srbm_rti_queued), K(srbm_rti_queued_logged)}, {K(srbm_rti_queued_long), K(srbm_rti_queued_long_logged)}}};
#undef K
    return table[queued][long_n][logged];
}
// ---- step log (srbm_steplog.hiph): the entries that log ask for room BEFORE they queue anything, so that a refused call leaves the batch untouched ----
static int log_room(const srbm_batch* h, const char* fn, int steps) {
    if (!h->d_log || steps <= h->log_cap - h->log_used) return 0;
    return fail(std::string(fn) + ": the step log has room for " + std::to_string(h->log_cap - h->log_used) + " more steps (" + std::to_string(h->log_used) +
                " of " + std::to_string(h->log_cap) + " logged), the call asks for " + std::to_string(steps) +
                " (srbm_step_log_reset, or srbm_step_log_enable with more steps)");
}
static SrbmStepLogArgs log_args(const srbm_batch* h) { return SrbmStepLogArgs{h->d_log, h->log_used, h->batch}; }
// the record of the one-step launch just queued (launch_step): its own small kernel behind the four phase kernels
static int log_one_step(srbm_batch* h) {
    if (!h->d_log) return 0;
    hipLaunchKernelGGL(srbm_k_step_log, dim3(h->batch), dim3(64), 0, h->stream, h->insts, h->d_state, h->d_time, h->d_ee, log_args(h));
    HIPCHK(hipGetLastError());
    h->log_used++;
    return 0;
}
// One RTI step on inputs already in h->d_state / d_time / d_ee: four kernels.  exact: the solve is taken to the gap criterion whatever the batch's
// step rule says (the solve whose KKT sensitivity the gait step differentiates).
// (Measured in round 5: the same step as ONE launch of the fused kernel -- no grid-wide wait between the phases, a workgroup through with its line-search
//  candidate takes the next one -- is SLOWER: gait segment 7.06 -> 7.34 ms per step; the stand-alone IPM kernel is an entry function -- its uniform
//  loads are scalar, it spills less (scratch 396 B per lane against 988) -- and that outweighs three kernel tails.)
static int launch_step(srbm_batch* h, bool exact = false) {
    if (upload_params(h)) return -1;
    // (start_mu only in the fused K-step launches: the lower-start attempt trades a shorter mean for a longer tail, and a one-step launch ends with
    //  the slowest instance of the batch -- srbm_k3_ipm.hiph)
    //  (Tried for the 10 x batch candidates of a gait line search, where dynamic workgroup scheduling evens out the tail: a candidate's linearisation
    //  point belongs to ANOTHER contact schedule -- 17-35 % of the attempts are repeated, the gait segment goes from 8.3 to 10.4-11.8 ms per step.)
    const double tol_step = exact ? 0.0 : h->hp.tol_step, start_mu = 0.0;
    h->last_tol_step = tol_step;
    const int B = h->batch;
    hipLaunchKernelGGL(srbm_k1_assemble, dim3(B), dim3(K1_THREADS), 0, h->stream, h->dp, h->insts, h->works, h->d_state, h->d_time, h->d_ee);
    hipLaunchKernelGGL(srbm_k2_condense, dim3(B), dim3(K2_THREADS), 0, h->stream, h->dp, h->insts, h->works);
    const bool tm = h->timing && h->ev_used < h->ev_start.size();
    if (tm) HIPCHK(hipEventRecord(h->ev_start[h->ev_used], h->stream));
    const auto k3 = k3_long(h) ? srbm_k3_ipm_long : srbm_k3_ipm;
    hipLaunchKernelGGL(k3, dim3(B), dim3(K3_THREADS), K3_LDS_LAUNCH_BYTES, h->stream, h->dp, h->insts, h->works, tol_step, start_mu);
    if (tm) { HIPCHK(hipEventRecord(h->ev_stop[h->ev_used], h->stream)); h->ev_steps[h->ev_used] = 1; h->ev_used++; }
    hipLaunchKernelGGL(srbm_k4_update, dim3(B), dim3(K4_THREADS), 0, h->stream, h->dp, h->insts, h->works);
    HIPCHK(hipGetLastError());
    return 0;
}

// The unit-test hooks of the dense blocks (srbm_dense_hooks.hiph): inputs in, the kernel on `count` workgroups with `lds` bytes of dynamic LDS,
// a device-wide wait, outputs back
template <class... P, class... A>
static int run_dense_hook(void (*kernel)(P...), int count, size_t lds, std::initializer_list<Copy> in, std::initializer_list<Copy> out, A... args) {
    if (copy_each(in, hipMemcpyHostToDevice)) return -1;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(count), dim3(DN_THREADS), lds, 0, args...);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return copy_each(out, hipMemcpyDeviceToHost);
}

extern "C" {

const char* srbm_last_error(void) { return g_err.c_str(); }
long srbm_bytes_per_instance(void) { return (long)(sizeof(SrbmInst) + sizeof(SrbmWork)); }
/* diagnostic builds (-DSRBM_PROFILE) only: the cycle record of one instance, srbm_debug_profile_slot(-1, ..) slots (srbm_prof.hiph) */
int srbm_debug_get_profile(srbm_batch* h, int inst, double* out) {
    if (!h || inst < 0 || inst >= h->batch || !out) return fail("bad arguments");
    return fetch(h, {{out, work_field(h, inst, offsetof(SrbmWork, prof)), sizeof(double) * SRBM_PROF_NSLOTS}});
}
/* the number of cycle slots; for 0 <= k below it, the printable name of slot k and of its group (the lists of srbm_prof.hiph) */
int srbm_debug_profile_slot(int k, const char** name, const char** group) {
#define SRBM_PROF_X_NAME(id, text) text,
#define SRBM_PROF_X_SLOT_NAME(grp, id, text) {text, SRBM_PROF_G_##grp},
    static const char* const groups[SRBM_PROF_NGROUPS] = { SRBM_PROF_GROUPS(SRBM_PROF_X_NAME) };
    static const struct { const char* name; int group; } slots[SRBM_PROF_NSLOTS] = { SRBM_PROF_SLOTS(SRBM_PROF_X_SLOT_NAME) };
    if (k >= 0 && k < SRBM_PROF_NSLOTS && name && group) { *name = slots[k].name; *group = groups[slots[k].group]; }
    return SRBM_PROF_NSLOTS;
}
/* the number of fields of a traced iteration, and in *iters the iterations srbm_debug_get_trace returns; for 0 <= k below it, the printable name of field k */
int srbm_debug_trace_field(int k, const char** name, int* iters) {
    static const char* const fields[SRBM_TRACE_NFIELDS] = { SRBM_TRACE_FIELDS(SRBM_PROF_X_NAME) };
    if (k >= 0 && k < SRBM_TRACE_NFIELDS && name) *name = fields[k];
    if (iters) *iters = SRBM_TRACE_ITERS;
    return SRBM_TRACE_NFIELDS;
}
/* unit-test hooks of the dense blocks (srbm_dense_hooks.hiph), in both builds: the packed matrices where the IPM keeps its normal matrix -- the
   LDS (standard build) or, SRBM_M_GLOBAL, a device workspace of one slice per matrix with DBG_PAD doubles after each --; `fill` is written to
   the doubles after each packed matrix (the LDS window's tail / the pad), which the helpers may read but whose values must not matter */
#ifdef SRBM_M_GLOBAL
#define DBG_WORKSPACE(tmp, Mw, np, count) HIPCHK((tmp).alloc(&(Mw), ((np) + DBG_PAD) * (count) * sizeof(double)))
#else
#define DBG_WORKSPACE(tmp, Mw, np, count) do { } while (0)
#endif
int srbm_debug_solve_mapped(int n, int nc, const int* map, int count, const double* M_packed, const double* rhs, double* x, int* nreg, double fill) {
    if (n <= 0 || n > SRBM_NUMAX || nc <= 0 || nc > n || count <= 0 || !map || !M_packed || !rhs || !x || !nreg) return fail("bad arguments");
    for (int k = 0; k < nc; k++) if (map[k] < 0 || map[k] >= n || (k > 0 && map[k] <= map[k - 1])) return fail("srbm_debug_solve_mapped: the map must be increasing and within [0, n)");
    const size_t np = (size_t)n * (n + 1) / 2, bytes = np * count * sizeof(double), vb = (size_t)n * count * sizeof(double);
    double *dM = nullptr, *dr = nullptr, *dx = nullptr, *Mw = nullptr; int *dmap = nullptr, *dn = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dM, bytes)); HIPCHK(tmp.alloc(&dr, vb)); HIPCHK(tmp.alloc(&dx, vb)); HIPCHK(tmp.alloc(&dmap, sizeof(int) * nc)); HIPCHK(tmp.alloc(&dn, sizeof(int) * count));
    DBG_WORKSPACE(tmp, Mw, np, count);
    return run_dense_hook(srbm_k_debug_solve_mapped, count, DbgLds::END * sizeof(double), {{dM, M_packed, bytes}, {dr, rhs, vb}, {dmap, map, sizeof(int) * nc}},
                          {{x, dx, vb}, {nreg, dn, sizeof(int) * count}}, n, nc, dmap, dM, dr, dx, dn, Mw, fill);
}
/* unit-test hook: x = M^-1 rhs through Cholesky + explicit inverse of the factor; X_packed = L^-1; ticks[2*count] */
int srbm_debug_solve(int n, int count, const double* M_packed, const double* rhs, double* x, double* X_packed, int* ticks, double fill) {
    if (n <= 0 || n > SRBM_NUMAX || count <= 0 || !M_packed || !rhs || !x || !X_packed || !ticks) return fail("bad arguments");
    const size_t np = (size_t)n * (n + 1) / 2, bytes = np * count * sizeof(double), vb = (size_t)n * count * sizeof(double);
    double *dM = nullptr, *dX = nullptr, *dr = nullptr, *dx = nullptr, *Mw = nullptr; int* dt = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dM, bytes)); HIPCHK(tmp.alloc(&dX, bytes)); HIPCHK(tmp.alloc(&dr, vb)); HIPCHK(tmp.alloc(&dx, vb));
    HIPCHK(tmp.alloc(&dt, sizeof(int) * 2 * count));
    DBG_WORKSPACE(tmp, Mw, np, count);
    return run_dense_hook(srbm_k_debug_solve, count, DbgLds::XC * sizeof(double), {{dM, M_packed, bytes}, {dr, rhs, vb}},
                          {{x, dx, vb}, {X_packed, dX, bytes}, {ticks, dt, sizeof(int) * 2 * count}}, n, dM, dr, dx, dX, dt, Mw, fill);
}
int srbm_debug_cholesky(int n, int count, const double* M_packed, double* L_packed, int* nreg, double fill) {
    if (n <= 0 || n > SRBM_NUMAX || count <= 0 || !M_packed || !L_packed || !nreg) return fail("bad arguments");
    const size_t np = (size_t)n * (n + 1) / 2, bytes = np * count * sizeof(double);
    double *dM = nullptr, *dL = nullptr, *Mw = nullptr; int* dr = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dM, bytes)); HIPCHK(tmp.alloc(&dL, bytes)); HIPCHK(tmp.alloc(&dr, sizeof(int) * count));
    DBG_WORKSPACE(tmp, Mw, np, count);
    return run_dense_hook(srbm_k_debug_cholesky, count, DbgLds::X * sizeof(double), {{dM, M_packed, bytes}}, {{L_packed, dL, bytes}, {nreg, dr, sizeof(int) * count}},
                          n, dM, dL, dr, Mw, fill);
}
/* unit-test hooks of the two mat-vecs of the IPM: y = H x for `count` packed symmetric n x n matrices H (lower triangle, row-major), through
   dn_sym_matvec with H where the IPM keeps its normal matrix, and through hmatvec_packed with H in global memory as SrbmWork::H */
int srbm_debug_sym_matvec(int n, int count, const double* H_packed, const double* xin, double* y) {
    if (n <= 0 || n > SRBM_NUMAX || count <= 0 || !H_packed || !xin || !y) return fail("bad arguments");
    const size_t np = (size_t)n * (n + 1) / 2, bytes = np * count * sizeof(double), vb = (size_t)n * count * sizeof(double);
    double *dH = nullptr, *dx = nullptr, *dy = nullptr, *Mw = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dH, bytes)); HIPCHK(tmp.alloc(&dx, vb)); HIPCHK(tmp.alloc(&dy, vb));
#ifdef SRBM_M_GLOBAL
    HIPCHK(tmp.alloc(&Mw, bytes));
#endif
    return run_dense_hook(srbm_k_debug_sym_matvec, count, DBG_SYM_MATVEC_LDS_BYTES, {{dH, H_packed, bytes}, {dx, xin, vb}}, {{y, dy, vb}}, n, dH, dx, dy, Mw);
}
int srbm_debug_hmatvec(int n, int count, const double* H_packed, const double* xin, double* y) {
    if (n <= 0 || n > SRBM_NUMAX || count <= 0 || !H_packed || !xin || !y) return fail("bad arguments");
    const size_t np = (size_t)n * (n + 1) / 2, bytes = np * count * sizeof(double), vb = (size_t)n * count * sizeof(double);
    double *dH = nullptr, *dx = nullptr, *dy = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dH, bytes)); HIPCHK(tmp.alloc(&dx, vb)); HIPCHK(tmp.alloc(&dy, vb));
    return run_dense_hook(srbm_k_debug_hmatvec, count, DBG_HMATVEC_LDS_BYTES, {{dH, H_packed, bytes}, {dx, xin, vb}}, {{y, dy, vb}}, n, dH, dx, dy);
}
/* unit-test hook of the IPM's staging of H (k3_load_h_o) and of the LDS map it publishes: `count` packed n x n matrices H, each into the H of a work
   record of its own, one workgroup of the IPM's launch shape each.  out[count][np + guard] <- the matrix of the solve and the `guard` (<= 64) doubles
   behind it after the staging, all of them set to the bit pattern 0xDEADBEEFCAFEF00D before it.  map5 (optional) [count][5] <- what an out-of-line phase reads
   of the map of a solve (N, n, wc): wc, rows in the tail of the matrix window, 1 if all rows are in LDS, offset of the tail rows, offset of the
   rows behind the map (doubles into the LDS) */
int srbm_debug_h_stage(int n, int count, const double* H_packed, double* out, int guard, int N, int wc, int* map5) {
    if (n <= 0 || n > SRBM_NUMAX || count <= 0 || !H_packed || !out || guard < 0 || guard > 64) return fail("bad arguments");
    if (map5 && (N < 4 || N > SRBM_NMAX || wc <= 0 || wc > K3_WCMAX)) return fail("bad arguments");
    const size_t np = (size_t)n * (n + 1) / 2, ob = (np + guard) * count * sizeof(double), mb = sizeof(int) * 5 * count;
    SrbmWork* dW = nullptr; double* dout = nullptr; int* dmap = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dW, sizeof(SrbmWork) * count)); HIPCHK(tmp.alloc(&dout, ob));
    if (map5) HIPCHK(tmp.alloc(&dmap, mb));
    for (int b = 0; b < count; b++) HIPCHK(hipMemcpy(dW[b].H, H_packed + b * np, np * sizeof(double), hipMemcpyHostToDevice));
    return run_dense_hook(srbm_k_debug_h_stage, count, K3_LDS_LAUNCH_BYTES, {}, {{out, dout, ob}, {map5, dmap, mb}}, n, dW, dout, guard, N, wc,
                          (int)(K3_LDS_LAUNCH_BYTES / sizeof(double)), dmap);
}
/* unit-test hook of the constant LDS base of the out-of-line device functions (SRBM_LDS_BASE, srbm_types.h), `count` workgroups: out4[count][4] <- the
   LDS address of the dynamic LDS as the kernel has it, the address an out-of-line function uses, the constant, and 0x5eed if a value the
   out-of-line function stored at double `slot` (< 64) of its dynamic LDS is read back by the kernel at the same slot of its own (0 otherwise) */
int srbm_debug_lds_base(int count, int slot, int* out4) {
    if (count <= 0 || slot < 0 || slot >= DBG_LDS_BASE_DOUBLES || !out4) return fail("bad arguments");
    unsigned* dout = nullptr;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&dout, sizeof(unsigned) * 4 * count));
    return run_dense_hook(srbm_k_debug_lds_base, count, DBG_LDS_BASE_DOUBLES * sizeof(double), {}, {{out4, dout, sizeof(unsigned) * 4 * count}}, slot, dout);
}
/* host only: where the IPM of this library puts the 2 (N - 3) compact dense state rows of width wc at n_u = nu (k3_sig_placement, the arithmetic of
   its LDS map): out3 = rows in the tail of the packed-matrix window, rows behind the LDS map, 1 if all are in LDS (0: read from L2) */
int srbm_debug_dense_row_placement(int N, int nu, int wc, int* out3) {
    if (N < 4 || N > SRBM_NMAX || nu <= 0 || nu > SRBM_NUMAX || wc <= 0 || wc > K3_WCMAX || !out3) return fail("bad arguments");
    const K3SigPlacement p = k3_sig_placement(N, nu, wc, (int)(K3_LDS_LAUNCH_BYTES / sizeof(double)));
    out3[0] = p.in_tail; out3[1] = p.in_extra; out3[2] = p.sig_lds;
    return 0;
}
// the trace of one instance, row by row: (iterations) x (fields) doubles, both numbers from srbm_debug_trace_field
int srbm_debug_get_trace(srbm_batch* h, int inst, double* out) {
    if (!h || inst < 0 || inst >= h->batch || !out) return fail("bad arguments");
    return fetch(h, {{out, work_field(h, inst, offsetof(SrbmWork, trace)), sizeof(SrbmWork::trace)}});
}

// diagnostic: the spline variables of the linearisation point and of the QP minimiser of instance `inst`, with the column descriptors
// (foot, type 0 force / 1 position, coordinate, local index) and the pin / substitution mask -- scripts/dev_attempts.py
int srbm_debug_get_spline_step(srbm_batch* h, int inst, double* u_prev, double* u, int* cols4, int* fix) {
    if (!h || inst < 0 || inst >= h->batch || !u_prev || !u || !cols4 || !fix) return fail("bad arguments");
    const size_t nd = sizeof(double) * SRBM_NUMAX, ni = sizeof(int) * SRBM_NUMAX;
    auto W = [&](size_t offset) { return work_field(h, inst, offset); };
    return fetch(h, {{u_prev, W(offsetof(SrbmWork, u_prev)), nd}, {u, W(offsetof(SrbmWork, u)), nd}, {cols4, W(offsetof(SrbmWork, col_ee)), ni},
                     {cols4 + SRBM_NUMAX, W(offsetof(SrbmWork, col_type)), ni}, {cols4 + 2 * SRBM_NUMAX, W(offsetof(SrbmWork, col_coord)), ni},
                     {cols4 + 3 * SRBM_NUMAX, W(offsetof(SrbmWork, col_local)), ni}, {fix, W(offsetof(SrbmWork, fix_mask)), ni}});
}

// diagnostic: what the condensing kernel left in the work record of instance `inst` at its last solve, at the capacities of this build -- H packed
// lower [NUMAX (NUMAX + 1) / 2], g [NUMAX], the compact dense state rows Sig [2 (NMAX - 3)][NUMAX], sig0 [2 (NMAX - 3)] -- with the instance's
// n_u and error bits (tests/test_gpu_condense.py, scripts/dev_bitwise_ab.py)
int srbm_debug_get_condensed(srbm_batch* h, int inst, double* H, double* g, double* Sig, double* sig0, int* nu, int* err) {
    if (!h || inst < 0 || inst >= h->batch || !H || !g || !Sig || !sig0 || !nu || !err) return fail("bad arguments");
    auto W = [&](size_t offset) { return work_field(h, inst, offset); };
    return fetch(h, {{H, W(offsetof(SrbmWork, H)), sizeof(SrbmWork::H)}, {g, W(offsetof(SrbmWork, g)), sizeof(SrbmWork::g)},
                     {Sig, W(offsetof(SrbmWork, Sig)), sizeof(SrbmWork::Sig)}, {sig0, W(offsetof(SrbmWork, sig0)), sizeof(SrbmWork::sig0)},
                     {nu, W(offsetof(SrbmWork, nu)), sizeof(int)}, {err, &h->insts[inst].err, sizeof(int)}});
}

// device buffers + kernel attributes of a batch whose host parameters (h->hp, batch, device) are set; on failure everything
// allocated so far is released by the caller through free_batch()
static void free_batch(srbm_batch* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->dp); (void)hipFree(h->insts); (void)hipFree(h->works); (void)hipFree(h->queues);
    (void)hipFree(h->d_state); (void)hipFree(h->d_time); (void)hipFree(h->d_ee);
    (void)hipFree(h->d_plant); (void)hipFree(h->d_push); (void)hipFree(h->d_period); (void)hipFree(h->d_dt);
    (void)hipFree(h->d_scratch); (void)hipFree(h->d_wbc); (void)hipHostFree(h->h_stage); (void)hipFree(h->d_log);
    (void)hipFree(h->d_sum); (void)hipFree(h->d_sum_ref);
    (void)hipFree(h->d_tick_q); (void)hipFree(h->d_tick_rec);
    (void)hipFree(h->d_wb); (void)hipFree(h->d_wb_int); (void)hipFree(h->d_tlog);
    (void)hipFree(h->d_tsum); (void)hipFree(h->d_tsum_ref);
    (void)hipFree(h->d_fd_act); (void)hipFree(h->d_fd_bodies);
    (void)hipFree(h->d_ground); (void)hipFree(h->d_terrain); (void)hipFree(h->d_cs); (void)hipFree(h->d_fb);
    (void)hipFree(h->pub_insts); (void)hipFree(h->d_lat); (void)hipFree(h->d_pub);
    (void)hipFree(h->d_sens); (void)hipFree(h->d_joints); (void)hipFree(h->d_wrench); (void)hipFree(h->d_cmd);
    for (auto e : h->ev_start) (void)hipEventDestroy(e);
    for (auto e : h->ev_stop) (void)hipEventDestroy(e);
    if (h->owns_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}
// the control tick's buffers (srbm_control_tick_reset, srbm_batch_clone)
static int tick_alloc(srbm_batch* h) {
    const size_t B = h->batch;
    if (!h->d_tick_q) HIPCHK(hipMalloc(&h->d_tick_q, sizeof(double) * 19 * B));
    if (!h->d_tick_rec) HIPCHK(hipMalloc(&h->d_tick_rec, sizeof(SrbmTickRec) * B));
    return 0;
}
// the buffers of the whole-controller rollout (srbm_wb_plant_set_state, srbm_batch_clone): per instance q[19], v[18], time[2] (ticks k and k + 1 in
// turn), control[36], qp_sol[30], state[13], ee[12]; status[2], contact[4]
enum { WB_DOUBLES = 19 + 18 + 2 + 36 + WBC_NMAX + 13 + 12, WB_INTS = 2 + 4 };
struct WbBuf { double *q, *v, *time, *control, *sol, *state, *ee; int *status, *contact; };
static WbBuf wb_buf(const srbm_batch* h) {
    const size_t B = h->batch;
    WbBuf w;
    w.q = h->d_wb; w.v = w.q + 19 * B; w.time = w.v + 18 * B; w.control = w.time + 2 * B; w.sol = w.control + 36 * B; w.state = w.sol + WBC_NMAX * B;
    w.ee = w.state + 13 * B;
    w.status = h->d_wb_int; w.contact = w.status + 2 * B;
    return w;
}
// the buffers of the sensor model, one allocation: per instance the device copy of the record, the state, the record of the run and the last
// measurement (qm, vm), then the seeds
struct SensBuf { double *S, *ms, *srec, *qm, *vm; unsigned long long* seed; };
enum { SENS_BUF_DOUBLES = SRBM_SENS_DEV_DOUBLES + SRBM_SENS_STATE_DOUBLES + SRBM_SENS_RECORD_DOUBLES + 19 + 18 };
static size_t sens_bytes(size_t B) { return sizeof(double) * SENS_BUF_DOUBLES * B + sizeof(unsigned long long) * B; }
static SensBuf sens_buf(const srbm_batch* h) {
    const size_t B = h->batch;
    SensBuf s;
    s.S = h->d_sens; s.ms = s.S + SRBM_SENS_DEV_DOUBLES * B; s.srec = s.ms + SRBM_SENS_STATE_DOUBLES * B; s.qm = s.srec + SRBM_SENS_RECORD_DOUBLES * B;
    s.vm = s.qm + 19 * B; s.seed = reinterpret_cast<unsigned long long*>(s.vm + 18 * B);
    return s;
}
// the buffers of the joint model, one allocation: the setting (joints, stops), the motor torques and the record
struct JointBuf { double *joints, *stops, *js, *jrec; };
enum { JOINT_BUF_DOUBLES = WBJ_INSTANCE_DOUBLES + WBJ_STOP_DOUBLES + 12 + WBJ_RECORD_DOUBLES };
static JointBuf joint_buf(const srbm_batch* h) {
    const size_t B = h->batch;
    JointBuf j;
    j.joints = h->d_joints; j.stops = j.joints + WBJ_INSTANCE_DOUBLES * B; j.js = j.stops + WBJ_STOP_DOUBLES * B; j.jrec = j.js + 12 * B;
    return j;
}
// the buffers of the wrench schedule, one allocation: the events and the record
enum { WRENCH_BUF_DOUBLES = WBW_INSTANCE_DOUBLES + WBW_RECORD_DOUBLES };
static SrbmWrenchArgs wrench_buf(const srbm_batch* h) { return SrbmWrenchArgs{h->d_wrench, h->d_wrench + WBW_INSTANCE_DOUBLES * (size_t)h->batch}; }
// the buffers of the command schedule, one allocation: the events, the state and the record
struct CmdBuf { double *cmds, *cstate, *crec; };
static size_t cmd_buf_doubles(const srbm_batch* h) { return ((size_t)h->cmd_events * CMD_EVENT_DOUBLES + CMD_STATE_DOUBLES + CMD_REC_DOUBLES) * (size_t)h->batch; }
static CmdBuf cmd_buf(const srbm_batch* h) {
    CmdBuf c;
    c.cmds = h->d_cmd; c.cstate = c.cmds + (size_t)h->cmd_events * CMD_EVENT_DOUBLES * h->batch; c.crec = c.cstate + CMD_STATE_DOUBLES * (size_t)h->batch;
    return c;
}
static int wb_alloc(srbm_batch* h) {
    const size_t B = h->batch;
    if (!h->d_wb) HIPCHK(hipMalloc(&h->d_wb, sizeof(double) * WB_DOUBLES * B));
    if (!h->d_wb_int) HIPCHK(hipMalloc(&h->d_wb_int, sizeof(int) * WB_INTS * B));
    if (!h->d_cs) HIPCHK(hipMalloc(&h->d_cs, sizeof(double) * WBG_CS_DOUBLES * B));
    if (!h->d_fb) HIPCHK(hipMalloc(&h->d_fb, sizeof(double) * SRBM_FB_DOUBLES * B));
    return 0;
}
static int alloc_batch(srbm_batch* h, hipStream_t borrowed_stream) {
    const size_t B = h->batch;
    if (borrowed_stream) { h->stream = borrowed_stream; h->owns_stream = false; }
    else { HIPCHK(hipStreamCreate(&h->stream)); h->owns_stream = true; }
    HIPCHK(hipMalloc(&h->dp, sizeof(SrbmParams) * B));
    HIPCHK(hipMalloc(&h->insts, sizeof(SrbmInst) * B));
    HIPCHK(hipMalloc(&h->works, sizeof(SrbmWork) * B));
    HIPCHK(hipMalloc(&h->d_state, sizeof(double) * 13 * B));
    HIPCHK(hipMalloc(&h->d_time, sizeof(double) * B));
    HIPCHK(hipMalloc(&h->d_ee, sizeof(double) * 12 * B));
    HIPCHK(hipMalloc(&h->d_dt, sizeof(double) * B));
    { const std::vector<double> dts(B, h->hp.dt); HIPCHK(hipMemcpy(h->d_dt, dts.data(), sizeof(double) * B, hipMemcpyHostToDevice)); }
    // the IPM kernel gets the whole LDS of a CU: what its fixed map leaves over holds the dense state rows (K3Smem::sig_row)
    if (srbm_k3_lds_bytes(h->hp.N) > K3_LDS_LAUNCH_BYTES) return fail("srbm_batch_create: LDS map exceeds 160 KB");
    h->hp.lds_doubles = (int)(K3_LDS_LAUNCH_BYTES / sizeof(double));
    // the kernels launched with dynamic LDS beyond the default limit, with the constant their launches pass
    const struct { const void* kernel; size_t lds; } dyn_lds[] = {
        {reinterpret_cast<const void*>(srbm_k3_ipm), K3_LDS_LAUNCH_BYTES},
        {reinterpret_cast<const void*>(srbm_k3_ipm_long), K3_LDS_LAUNCH_BYTES},
        {reinterpret_cast<const void*>(srbm_k3_normal_matrix), K3_LDS_LAUNCH_BYTES},
        {reinterpret_cast<const void*>(srbm_k_gait_sensitivity), KG_DYN_LDS_BYTES}};
    for (const auto& k : dyn_lds) HIPCHK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
    for (int i = 0; i < 8; i++)
        HIPCHK(hipFuncSetAttribute(multi_step_kernel(i & 4, i & 2, i & 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)K3_LDS_LAUNCH_BYTES));
    HIPCHK(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    { const char* e = std::getenv("SRBM_NO_STEP_QUEUE"); h->queued_ok = !(e && e[0] == '1'); }
    h->params_dirty = true;
    return 0;
}

// The checks of srbm_batch_create / srbm_batch_create_each, before any device is probed (so that they can be tested without a GPU).  each: info and
// model are arrays [batch], else one record for every instance.  The fields that fix the QP shapes, the LDS map, the time grid and the foot geometry
// are batch-wide: instances that disagree on one are refused with its name.
static int check_create(const char* fn, srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, bool each) {
    if (!out || !info || !model || batch <= 0) return fail(std::string(fn) + ": bad arguments");
    if (info->num_nodes < 5 || info->num_nodes > SRBM_NMAX) return fail(std::string(fn) + ": num_nodes must be in [5, " + std::to_string(SRBM_NMAX) + "]");
    for (int b = 1; each && b < batch; b++) {
        const srbm_mpc_info& a = info[b];
        const char* field = a.num_nodes != info->num_nodes ? "num_nodes" : a.integrator_dt != info->integrator_dt ? "integrator_dt"
                          : a.swing_height != info->swing_height ? "swing_height" : a.foot_offset != info->foot_offset ? "foot_offset"
                          : std::memcmp(model[b].hip_xy, model->hip_xy, sizeof(model->hip_xy)) != 0 ? "hip_xy" : nullptr;
        if (field) return fail(std::string(fn) + ": instance " + std::to_string(b) + ": " + field + " differs from instance 0 (it is batch-wide: one value "
                               "for every instance of a batch)");
    }
    return 0;
}
static void set_inst_model(InstModel& m, const srbm_mpc_info& info, const srbm_model& model) {
    m.mu_fric = info.friction_coef; m.force_bound = info.force_bound; m.force_cost = info.force_cost;
    m.box0[0] = info.ee_box_size[0]; m.box0[1] = info.ee_box_size[1];
    m.mass = model.mass;
    std::memcpy(m.Ir, model.Ir, sizeof(m.Ir));
    inv3(m.Ir, m.Ir_inv);
}
static int create_batch(srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, bool each, int device) {
    const char* fn = each ? "srbm_batch_create_each" : "srbm_batch_create";
    if (check_create(fn, out, batch, info, model, each)) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(std::string(fn) + ": no HIP device (this library has no CPU path)");
    HIPCHK(hipSetDevice(device));
    auto* h = new srbm_batch;
    h->batch = batch; h->device = device;
    SrbmParams& p = h->hp;
    std::memset(&p, 0, sizeof(p));
    p.batch = batch; p.N = info->num_nodes; p.max_iter = 200;
    p.dt = info->integrator_dt; p.swing_height = info->swing_height; p.foot_offset = info->foot_offset;
    h->im.resize(batch);
    for (int b = 0; b < batch; b++) {
        InstModel& m = h->im[b];
        std::memset(&m, 0, sizeof(m));
        set_inst_model(m, info[each ? b : 0], model[each ? b : 0]);
    }
    std::memcpy(h->hip_xy, model->hip_xy, sizeof(h->hip_xy));
    for (int ee = 0; ee < 4; ee++) {      // GetCOMToHip, single_rigid_body_model.cpp:289-305
        double x = model->hip_xy[2 * ee], y = model->hip_xy[2 * ee + 1];
        if (y >= 0) y += 0.1; else y -= 0.1;
        x += 0.025;
        p.hip[2 * ee] = x; p.hip[2 * ee + 1] = y;
    }
    p.merit_mu = 5000; p.td_fraction = 0.75;
    // ClarabelInterface::ConfigureForInitialRun / ConfigureForRealTime (clarabel_interface.cpp:165-175) run every solve of the
    // reference at tol_gap 1e-15, tol_feas 1e-10: the defaults here.  The gap of this QP stops improving around 1e-14..1e-15
    // in fp64 (the loop then ends on its progress test), but WHERE it stops decides how well the minimiser is determined along
    // the flat directions of the weakly convex QP: measured against the CPU restatement of the reference on identical QPs (scripts/dev_accuracy.py,
    // 1024 solves) the worst relative primal error is 1.3e-4 at 1e-13, 5e-5 at 1e-14 and 1.4e-5 at 1e-15, for 17.3 / 18.0 /
    // 18.9 IPM iterations per solve.  The parity tolerance of the path is 1e-4.  srbm_set_solver_tolerances overrides.
    p.tol_gap_abs = 1e-15; p.tol_gap_rel = 1e-15; p.tol_feas = 1e-10;
    p.tol_step = 0.0; p.start_mu = 0.0;       // the reference's criterion; srbm_set_solver_step_rule opts into the faster termination
    auto bail = [&]() { free_batch(h); return -1; };
    if (alloc_batch(h, nullptr)) return bail();
    if (hipMemsetAsync(h->works, 0, sizeof(SrbmWork) * (size_t)batch, h->stream) != hipSuccess) { fail(std::string(fn) + ": memset failed"); return bail(); }
    if (upload_params(h)) return bail();
    hipLaunchKernelGGL(srbm_k_init, dim3((batch + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { fail(std::string(fn) + ": initialisation kernel failed"); return bail(); }
    *out = h;
    return 0;
}
int srbm_batch_create(srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, int device) {
    return create_batch(out, batch, info, model, false, device);
}
int srbm_batch_create_each(srbm_batch** out, int batch, const srbm_mpc_info* info, const srbm_model* model, int device) {
    return create_batch(out, batch, info, model, true, device);
}
int srbm_get_instance_model(const srbm_batch* h, int inst, srbm_mpc_info* info, srbm_model* model) {
    if (!h || inst < 0 || inst >= h->batch || !info || !model) return fail("srbm_get_instance_model: bad arguments");
    const InstModel& m = h->im[inst];
    info->num_nodes = h->hp.N; info->integrator_dt = h->hp.dt; info->friction_coef = m.mu_fric; info->force_bound = m.force_bound;
    info->swing_height = h->hp.swing_height; info->foot_offset = h->hp.foot_offset;
    info->ee_box_size[0] = m.box0[0]; info->ee_box_size[1] = m.box0[1]; info->force_cost = m.force_cost;
    model->mass = m.mass;
    std::memcpy(model->Ir, m.Ir, sizeof(model->Ir));
    std::memcpy(model->hip_xy, h->hip_xy, sizeof(model->hip_xy));
    return 0;
}

// MPC::MPC(const MPC&) (mpc.cpp:1133-1181): a deep copy with its own stream and buffers
int srbm_batch_clone(const srbm_batch* src, srbm_batch** out) {
    if (!src || !out) return fail("srbm_batch_clone: bad arguments");
    HIPCHK(hipSetDevice(src->device));
    HIPCHK(hipStreamSynchronize(src->stream));
    auto* h = new srbm_batch;
    h->batch = src->batch; h->device = src->device; h->hp = src->hp; h->im = src->im; std::memcpy(h->hip_xy, src->hip_xy, sizeof(h->hip_xy));
    h->push_set = src->push_set; h->last_tol_step = src->last_tol_step; h->period = src->period;
    auto bail = [&]() { free_batch(h); return -1; };
    if (alloc_batch(h, nullptr)) return bail();
    const size_t B = h->batch;
    auto cp = [&](void* d, const void* s_, size_t n) { return hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToDevice, h->stream) == hipSuccess; };
    bool ok = cp(h->insts, src->insts, sizeof(SrbmInst) * B) && cp(h->works, src->works, sizeof(SrbmWork) * B) &&
              cp(h->d_state, src->d_state, sizeof(double) * 13 * B) && cp(h->d_time, src->d_time, sizeof(double) * B) &&
              cp(h->d_ee, src->d_ee, sizeof(double) * 12 * B);
    if (ok && src->d_plant) {
        ok = hipMalloc(&h->d_plant, sizeof(double) * 13 * B) == hipSuccess && hipMalloc(&h->d_push, sizeof(double) * SRBM_PUSH_DOUBLES * B) == hipSuccess &&
             cp(h->d_plant, src->d_plant, sizeof(double) * 13 * B) && cp(h->d_push, src->d_push, sizeof(double) * SRBM_PUSH_DOUBLES * B);
    }
    if (ok && src->d_period) ok = hipMalloc(&h->d_period, sizeof(double) * B) == hipSuccess && cp(h->d_period, src->d_period, sizeof(double) * B);
    if (ok && src->d_wbc) ok = hipMalloc(&h->d_wbc, sizeof(SrbmWbcParams)) == hipSuccess && cp(h->d_wbc, src->d_wbc, sizeof(SrbmWbcParams));      // (a clone carries the complete state)
    // (the control tick's q_des_ goes along)
    if (ok && src->d_tick_q) ok = tick_alloc(h) == 0 && cp(h->d_tick_q, src->d_tick_q, sizeof(double) * 19 * B);
    // (... and the whole-body plant's (q, v); the tick log, like the step log, stays off)
    if (ok && src->d_wb) ok = wb_alloc(h) == 0 && cp(h->d_wb, src->d_wb, sizeof(double) * (19 + 18) * B) && cp(h->d_cs, src->d_cs, sizeof(double) * WBG_CS_DOUBLES * B);
    // (... and the contact-feedback setting with its record)
    h->contact_fb = src->contact_fb;
    if (ok && src->d_wb) ok = cp(h->d_fb, src->d_fb, sizeof(double) * SRBM_FB_DOUBLES * B);
    // (... and the kind of the plant, its actuators, sub-steps and bodies)
    h->fd_kind = src->fd_kind; h->fd_substeps = src->fd_substeps;
    if (ok && src->d_fd_act)
        ok = hipMalloc(&h->d_fd_act, sizeof(double) * WBFD_ACT_DOUBLES * B) == hipSuccess && cp(h->d_fd_act, src->d_fd_act, sizeof(double) * WBFD_ACT_DOUBLES * B);
    if (ok && src->d_fd_bodies)
        ok = hipMalloc(&h->d_fd_bodies, sizeof(SrbmBody) * 13 * B) == hipSuccess && cp(h->d_fd_bodies, src->d_fd_bodies, sizeof(SrbmBody) * 13 * B);
    // (... and its ground; the contact state went with (q, v))
    if (ok && src->d_ground)
        ok = hipMalloc(&h->d_ground, sizeof(double) * WBG_GROUND_DOUBLES * B) == hipSuccess && cp(h->d_ground, src->d_ground, sizeof(double) * WBG_GROUND_DOUBLES * B);
    // (... and the ground's terrain)
    h->terrain_patches = src->terrain_patches;
    if (ok && src->d_terrain)
        ok = hipMalloc(&h->d_terrain, sizeof(double) * WBT_INSTANCE_DOUBLES * B) == hipSuccess && cp(h->d_terrain, src->d_terrain, sizeof(double) * WBT_INSTANCE_DOUBLES * B);
    // (... and the latency setting with the published trajectories and the latency record)
    h->lat = src->lat; h->pub_init = src->pub_init;
    if (ok && src->pub_insts)
        ok = hipMalloc(&h->pub_insts, sizeof(SrbmInst) * B) == hipSuccess && hipMalloc(&h->d_lat, sizeof(double) * SRBM_LAT_DOUBLES * B) == hipSuccess &&
             hipMalloc(&h->d_pub, sizeof(double) * SRBM_PUB_DOUBLES * B) == hipSuccess && cp(h->pub_insts, src->pub_insts, sizeof(SrbmInst) * B) &&
             cp(h->d_lat, src->d_lat, sizeof(double) * SRBM_LAT_DOUBLES * B) && cp(h->d_pub, src->d_pub, sizeof(double) * SRBM_PUB_DOUBLES * B);
    // (... and the sensor setting with the sensor state, its record and the last measurement)
    h->sens = src->sens; h->sens_seed = src->sens_seed; h->sens_ready = src->sens_ready;
    if (ok && src->d_sens) ok = hipMalloc(&h->d_sens, sens_bytes(B)) == hipSuccess && cp(h->d_sens, src->d_sens, sens_bytes(B));
    // (... and the joint model with the motor torques and its record)
    h->joints = src->joints;
    if (ok && src->d_joints)
        ok = hipMalloc(&h->d_joints, sizeof(double) * JOINT_BUF_DOUBLES * B) == hipSuccess && cp(h->d_joints, src->d_joints, sizeof(double) * JOINT_BUF_DOUBLES * B);
    // (... and the wrench schedule with its record)
    h->wrenches = src->wrenches; h->wrench_events = src->wrench_events;
    if (ok && src->d_wrench)
        ok = hipMalloc(&h->d_wrench, sizeof(double) * WRENCH_BUF_DOUBLES * B) == hipSuccess && cp(h->d_wrench, src->d_wrench, sizeof(double) * WRENCH_BUF_DOUBLES * B);
    // (... and the command schedule with its state and record)
    h->cmds = src->cmds; h->cmd_init = src->cmd_init; h->cmd_events = src->cmd_events;
    if (ok && src->d_cmd)
        ok = hipMalloc(&h->d_cmd, sizeof(double) * cmd_buf_doubles(src)) == hipSuccess && cp(h->d_cmd, src->d_cmd, sizeof(double) * cmd_buf_doubles(src));
    if (!ok) { fail("srbm_batch_clone: device copy failed"); return bail(); }
    if (upload_params(h)) return bail();
    if (hipStreamSynchronize(h->stream) != hipSuccess) { fail("srbm_batch_clone: synchronisation failed"); return bail(); }
    *out = h;
    return 0;
}
int srbm_get_capacity(int* cap4) { if (!cap4) return fail("bad arguments"); cap4[0] = SRBM_NMAX; cap4[1] = SRBM_NUMAX; cap4[2] = SRBM_NSMAX; cap4[3] = SRBM_KMAX; return 0; }
int srbm_batch_size(const srbm_batch* h) { return h ? h->batch : -1; }
int srbm_num_nodes(const srbm_batch* h) { return h ? h->hp.N : -1; }

int srbm_batch_destroy(srbm_batch* h) {
    if (!h) return 0;
    if (h->gait_refs > 0) return fail("srbm_batch_destroy: srbm_gait handles still borrow this batch (destroy them first)");
    free_batch(h);
    return 0;
}

// The cost setters write instances [first, first + count) from arrays [count][...]; the batch-wide entries below write every instance (the last write
// wins per instance).
static int check_each(const char* fn, const srbm_batch* h, int first, int count, std::initializer_list<const void*> arrays) {
    if (!h) return fail(std::string(fn) + ": bad arguments (NULL handle)");
    if (first < 0 || count < 0 || first > h->batch || count > h->batch - first)
        return fail(std::string(fn) + ": first / count out of range (first " + std::to_string(first) + ", count " + std::to_string(count) + ", batch " +
                    std::to_string(h->batch) + ")");
    for (const void* a : arrays) if (!a) return fail(std::string(fn) + ": bad arguments (NULL array)");
    return 0;
}
static void tracking_cost(InstModel& m, const double* state_des12, const double* Q144) {
    std::memcpy(m.Q, Q144, sizeof(double) * 144);
    for (int i = 0; i < 12; i++) {
        double a = 0;
        for (int j = 0; j < 12; j++) a += Q144[i * 12 + j] * state_des12[j];
        m.w[i] = -1 * a;
    }
}
int srbm_add_quadratic_tracking_cost_each(srbm_batch* h, int first, int count, const double* state_des12, const double* Q144) {
    if (check_each("srbm_add_quadratic_tracking_cost_each", h, first, count, {state_des12, Q144})) return -1;
    for (int i = 0; i < count; i++) tracking_cost(h->im[first + i], state_des12 + 12 * i, Q144 + 144 * i);
    params_changed(h);
    return 0;
}
int srbm_set_quadratic_final_cost_each(srbm_batch* h, int first, int count, const double* Phi144) {
    if (check_each("srbm_set_quadratic_final_cost_each", h, first, count, {Phi144})) return -1;
    for (int i = 0; i < count; i++) std::memcpy(h->im[first + i].Phi, Phi144 + 144 * i, sizeof(double) * 144);
    params_changed(h);
    return 0;
}
int srbm_set_linear_final_cost_each(srbm_batch* h, int first, int count, const double* w12) {
    if (check_each("srbm_set_linear_final_cost_each", h, first, count, {w12})) return -1;
    for (int i = 0; i < count; i++) std::memcpy(h->im[first + i].Phi_w, w12 + 12 * i, sizeof(double) * 12);
    params_changed(h);
    return 0;
}
int srbm_add_force_cost_each(srbm_batch* h, int first, int count, const double* weight) {
    if (check_each("srbm_add_force_cost_each", h, first, count, {weight})) return -1;
    for (int i = 0; i < count; i++) h->im[first + i].force_cost = weight[i];
    params_changed(h);
    return 0;
}
int srbm_add_quadratic_tracking_cost(srbm_batch* h, const double* state_des12, const double* Q144) {
    if (!h || !state_des12 || !Q144) return fail("bad arguments");
    for (InstModel& m : h->im) tracking_cost(m, state_des12, Q144);
    params_changed(h);
    return 0;
}
int srbm_set_quadratic_final_cost(srbm_batch* h, const double* Phi144) {
    if (!h || !Phi144) return fail("bad arguments");
    for (InstModel& m : h->im) std::memcpy(m.Phi, Phi144, sizeof(double) * 144);
    params_changed(h);
    return 0;
}
int srbm_set_linear_final_cost(srbm_batch* h, const double* w12) {
    if (!h || !w12) return fail("bad arguments");
    for (InstModel& m : h->im) std::memcpy(m.Phi_w, w12, sizeof(double) * 12);
    params_changed(h);
    return 0;
}
// MPC::AddForceCost (mpc.cpp:791-802): weight on every force spline variable
int srbm_add_force_cost(srbm_batch* h, double weight) {
    if (!h) return fail("bad arguments");
    for (InstModel& m : h->im) m.force_cost = weight;
    params_changed(h);
    return 0;
}
int srbm_set_solver_tolerances(srbm_batch* h, double ga, double gr, double tf, int max_iter) {
    if (!h) return fail("bad arguments");
    h->hp.tol_gap_abs = ga; h->hp.tol_gap_rel = gr; h->hp.tol_feas = tf; h->hp.max_iter = max_iter;
    params_changed(h);
    return 0;
}
int srbm_set_solver_step_rule(srbm_batch* h, double tol_step, double start_mu) {
    if (!h || !(tol_step >= 0.0) || !(start_mu >= 0.0)) return fail("bad arguments");
    h->hp.tol_step = tol_step; h->hp.start_mu = start_mu;
    params_changed(h);
    return 0;
}
int srbm_get_solver_step_rule(const srbm_batch* h, double* tol_step, double* start_mu) {
    if (!h || !tol_step || !start_mu) return fail("bad arguments");
    *tol_step = h->hp.tol_step; *start_mu = h->hp.start_mu;
    return 0;
}
int srbm_set_state_trajectory_warm_start(srbm_batch* h, const double* states) {
    if (!h || !states) return fail("bad arguments");
    if (use_batch(h)) return -1;
    HIPCHK(hipMemcpyAsync(h->d_state, states, sizeof(double) * 13 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(srbm_k_warm_start, dim3(h->batch), dim3(64), 0, h->stream, h->dp, h->insts, h->d_state);
    HIPCHK(hipGetLastError());
    return srbm_synchronize(h);
}

static int upload_inputs(srbm_batch* h, const double* state, const double* init_time, const double* ee) {
    const size_t B = h->batch;
    HIPCHK(hipMemcpyAsync(h->d_state, state, sizeof(double) * 13 * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ee, ee, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream));
    if (init_time) HIPCHK(hipMemcpyAsync(h->d_time, init_time, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(hipMemsetAsync(h->d_time, 0, sizeof(double) * B, h->stream));
    return 0;
}

int srbm_create_initial_run(srbm_batch* h, const double* state, const double* ee) {
    if (!h || !state || !ee) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (upload_inputs(h, state, nullptr, ee)) return -1;
    for (int it = 0; it < 10; it++) if (launch_step(h)) return -1;     // mpc.cpp:85-88: always 10 solves
    return srbm_synchronize(h);
}
int srbm_get_real_time_update(srbm_batch* h, const double* state, const double* init_time, const double* ee) {
    if (!h || !state || !init_time || !ee) return fail("bad arguments");
    if (log_room(h, "srbm_get_real_time_update", 1)) return -1;
    HIPCHK(hipSetDevice(h->device));
    if (upload_inputs(h, state, init_time, ee)) return -1;
    if (launch_step(h) || log_one_step(h)) return -1;
    return srbm_synchronize(h);
}
int srbm_get_real_time_update_dev(srbm_batch* h, const double* state_dev, const double* time_dev, const double* ee_dev) {
    if (!h || !state_dev || !time_dev || !ee_dev) return fail("bad arguments");
    if (log_room(h, "srbm_get_real_time_update_dev", 1)) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    HIPCHK(hipMemcpyAsync(h->d_state, state_dev, sizeof(double) * 13 * B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ee, ee_dev, sizeof(double) * 12 * B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_time, time_dev, sizeof(double) * B, hipMemcpyDeviceToDevice, h->stream));
    return launch_step(h) || log_one_step(h) ? -1 : 0;
}
static int launch_fused(srbm_batch* h, const char* fn, int first_index, int steps, SrbmPlantArgs pl) {
    if (log_room(h, fn, steps)) return -1;
    // (the lower-start attempt rests on the linearisation point being close to the new minimiser: true for the open-loop protocol, whose state IS
    //  node 1 of the plan; under a plant -- integration error every step, pushes -- it is repeated too often to pay: closed loop 62 k it/s with, 80 k without)
    pl.tol_step = h->hp.tol_step; pl.start_mu = pl.plant ? 0.0 : h->hp.start_mu;
    if (use_batch(h)) return -1;
    if (steps == 0) return 0;
    h->last_tol_step = pl.tol_step;
    // one launch for all steps (double time = i*info.integrator_dt, gait_opt_playground.cpp:84, is formed on the device)
    const bool tm = h->timing && h->ev_used < h->ev_start.size();
    if (tm) HIPCHK(hipEventRecord(h->ev_start[h->ev_used], h->stream));
    // a batch larger than the chip, several steps: a resident grid takes (instance, step) items from the step queues (srbm_fused.hiph)
    const bool queued = h->queued_ok && h->batch > h->n_cu && steps > 1 && steps <= SRBM_QUEUE_MAX_STEPS && h->batch <= SRBM_QUEUE_MAX_BATCH;
    const bool long_n = k3_long(h);
    h->last_launch_kernel = (queued ? 3 : 1) + (long_n ? 1 : 0);          // the codes of srbm_debug_get_launch_info (a logged launch: its unlogged twin's)
    h->last_launch_steps = steps;
    const bool logged = h->d_log != nullptr;                              // the logged twin of the same kernel: step s to slot log_used + s
    if (queued) {
        if (!h->queues) HIPCHK(hipMalloc(&h->queues, sizeof(SrbmQueue) * SRBM_NQUEUES));
        hipLaunchKernelGGL(srbm_k_queue_init, dim3(SRBM_NQUEUES), dim3(256), 0, h->stream, h->queues, h->batch);
    }
    // one workgroup per instance, or (step queues) a resident grid of one workgroup per CU; the argument list of the kernel chosen (multi_step_kernel)
    SrbmStepLogArgs lg = log_args(h);
    void* args[12] = {&h->dp, &h->insts, &h->works, &first_index, &steps, &h->d_state, &h->d_time, &h->d_ee, &pl};
    int na = 9;
    if (queued) { args[na++] = &h->queues; args[na++] = &h->batch; }
    if (logged) args[na++] = &lg;
    (void)hipLaunchKernel(multi_step_kernel(queued, long_n, logged), dim3(queued ? h->n_cu : h->batch), dim3(K3_THREADS), args, K3_LDS_LAUNCH_BYTES,
                          h->stream);          // (its error, if any, is the one hipGetLastError reports below)
    if (logged) h->log_used += steps;
    if (tm) { HIPCHK(hipEventRecord(h->ev_stop[h->ev_used], h->stream)); h->ev_steps[h->ev_used] = steps; h->ev_used++; }
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_rti_advance(srbm_batch* h, int first_index, int steps) {
    if (!h || steps < 0) return fail("bad arguments");
    return launch_fused(h, "srbm_rti_advance", first_index, steps, SrbmPlantArgs{nullptr, nullptr, h->d_dt, 1, 0, 0.0, 0.0});
}

// ---- closed-loop rollout harness (srbm_plant.hiph) ----
static int plant_alloc(srbm_batch* h) {
    if (h->d_plant) return 0;
    const size_t B = h->batch;
    HIPCHK(hipMalloc(&h->d_plant, sizeof(double) * 13 * B));
    HIPCHK(hipMalloc(&h->d_push, sizeof(double) * SRBM_PUSH_DOUBLES * B));
    HIPCHK(hipMemsetAsync(h->d_push, 0, sizeof(double) * SRBM_PUSH_DOUBLES * B, h->stream));          // (a clone copies it whether a push is set or not)
    return 0;
}
int srbm_plant_set_state(srbm_batch* h, const double* state) {
    if (!h || !state) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (plant_alloc(h)) return -1;
    HIPCHK(hipMemcpyAsync(h->d_plant, state, sizeof(double) * 13 * h->batch, hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_plant_get_state(srbm_batch* h, double* state) {
    if (!h || !state) return fail("bad arguments");
    if (!h->d_plant) return fail("the plant state has not been set (srbm_plant_set_state)");
    return fetch(h, {{state, h->d_plant, sizeof(double) * 13 * h->batch}});
}
int srbm_plant_set_push(srbm_batch* h, const double* time, const double* impulse) {
    if (!h || (time == nullptr) != (impulse == nullptr)) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (plant_alloc(h)) return -1;
    h->push_set = time != nullptr;
    if (time) {
        std::vector<double> rec((size_t)SRBM_PUSH_DOUBLES * h->batch);          // one record {time, impulse[6]} per instance
        for (int b = 0; b < h->batch; b++) {
            rec[(size_t)b * SRBM_PUSH_DOUBLES] = time[b];
            std::memcpy(&rec[(size_t)b * SRBM_PUSH_DOUBLES + 1], impulse + (size_t)b * 6, sizeof(double) * 6);
        }
        HIPCHK(hipMemcpyAsync(h->d_push, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));          // (rec leaves scope)
    }
    return 0;
}
// the MPC period of the closed-loop protocols, per instance; the open-loop entries never see it (their SrbmPlantArgs carry the array of dt)
int srbm_plant_set_period(srbm_batch* h, const double* period) {
    if (!h) return fail("srbm_plant_set_period: bad arguments (NULL handle)");
    if (!period) { h->period.clear(); return 0; }          // (the device array stays allocated; the launches are handed the array of dt)
    const double horizon = h->hp.N * h->hp.dt;
    for (int b = 0; b < h->batch; b++)
        if (!std::isfinite(period[b]) || period[b] <= 0.0 || period[b] >= horizon) {
            char v[64]; std::snprintf(v, sizeof v, "%.17g", period[b]);
            return fail("srbm_plant_set_period: the period of instance " + std::to_string(b) + " is " + v + ": a finite period in (0, num_nodes * dt = " +
                        std::to_string(horizon) + ") is required (beyond it the plant would read past the trajectory)");
        }
    HIPCHK(hipSetDevice(h->device));
    if (!h->d_period) HIPCHK(hipMalloc(&h->d_period, sizeof(double) * h->batch));
    HIPCHK(hipMemcpyAsync(h->d_period, period, sizeof(double) * h->batch, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->period.assign(period, period + h->batch);
    return 0;
}
int srbm_plant_get_period(srbm_batch* h, double* period) {
    if (!h || !period) return fail("srbm_plant_get_period: bad arguments");
    for (int b = 0; b < h->batch; b++) period[b] = h->period.empty() ? h->hp.dt : h->period[b];
    return 0;
}
// the plant arguments of a closed-loop launch
static SrbmPlantArgs plant_args(const srbm_batch* h, int substeps, int advance_time) {
    return SrbmPlantArgs{h->d_plant, h->push_set ? h->d_push : nullptr, h->period.empty() ? h->d_dt : h->d_period, substeps, advance_time ? 1 : 0};
}
int srbm_closed_loop_advance(srbm_batch* h, int first_index, int steps, int substeps, int advance_time) {
    if (!h || steps < 0 || substeps < 1) return fail("bad arguments");
    if (!h->d_plant) return fail("the plant state has not been set (srbm_plant_set_state)");
    return launch_fused(h, "srbm_closed_loop_advance", first_index, steps, plant_args(h, substeps, advance_time));
}
// the same protocol, one kernel launch per phase and step (grid-wide synchronisation between the phases); kept for
// A/B measurements against the fused kernel
int srbm_rti_advance_unfused(srbm_batch* h, int first_index, int steps) {
    if (!h || steps < 0) return fail("bad arguments");
    if (log_room(h, "srbm_rti_advance_unfused", steps)) return -1;
    if (use_batch(h)) return -1;
    for (int i = 0; i < steps; i++) {
        const double time = (first_index + i) * h->hp.dt;
        hipLaunchKernelGGL(srbm_k_next_inputs, dim3(h->batch), dim3(64), 0, h->stream, h->dp, h->insts, time, h->d_state, h->d_time, h->d_ee);
        if (launch_step(h) || log_one_step(h)) return -1;
    }
    return 0;
}

// ---- the step log (include/srbm_rti.h; csrc/srbm_steplog.hiph) ----
int srbm_step_log_record_doubles(void) { return SRBM_STEP_LOG_DOUBLES; }
int srbm_step_log_enable(srbm_batch* h, int max_steps) {
    if (!h || max_steps < 0) return fail("srbm_step_log_enable: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_log) HIPCHK(hipFree(h->d_log));
    h->d_log = nullptr; h->log_cap = 0; h->log_used = 0;
    if (max_steps == 0) return 0;
    const size_t bytes = sizeof(double) * SRBM_STEP_LOG_DOUBLES * (size_t)h->batch * (size_t)max_steps;
    HIPCHK(hipMalloc(&h->d_log, bytes));
    h->log_cap = max_steps;
    return 0;
}
int srbm_step_log_reset(srbm_batch* h) {
    if (!h) return fail("srbm_step_log_reset: bad arguments");
    h->log_used = 0;
    return 0;
}
int srbm_step_log_count(srbm_batch* h, int* steps_logged) {
    if (!h || !steps_logged) return fail("srbm_step_log_count: bad arguments");
    *steps_logged = h->log_used;
    return 0;
}
// the device address of slots [first_slot, first_slot + count) once the range is known to be logged
static int log_range(const srbm_batch* h, const char* fn, int first_slot, int count, const void* out, const double** src, size_t* bytes) {
    if (!h || !out) return fail(std::string(fn) + ": bad arguments");
    if (!h->d_log) return fail(std::string(fn) + ": no step log is enabled on this batch (srbm_step_log_enable)");
    if (first_slot < 0 || count < 0 || first_slot > h->log_used || count > h->log_used - first_slot)
        return fail(std::string(fn) + ": slots [" + std::to_string(first_slot) + ", " + std::to_string((long long)first_slot + count) + ") are outside the " +
                    std::to_string(h->log_used) + " steps logged");
    const size_t rec = (size_t)SRBM_STEP_LOG_DOUBLES * h->batch;
    *src = h->d_log + rec * first_slot;
    *bytes = sizeof(double) * rec * count;
    return 0;
}
int srbm_step_log_get(srbm_batch* h, int first_slot, int count, double* out) {
    const double* src = nullptr; size_t bytes = 0;
    if (log_range(h, "srbm_step_log_get", first_slot, count, out, &src, &bytes)) return -1;
    if (bytes == 0) return 0;
    return fetch(h, {{out, src, bytes}});
}
int srbm_step_log_copy_dev(srbm_batch* h, int first_slot, int count, double* out_dev) {
    const double* src = nullptr; size_t bytes = 0;
    if (log_range(h, "srbm_step_log_copy_dev", first_slot, count, out_dev, &src, &bytes)) return -1;
    if (bytes == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out_dev, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
// ---- rollout summaries (include/srbm_rti.h; csrc/srbm_rollout_summary.hiph) ----
int srbm_rollout_summary_doubles(void) { return SRBM_ROLLOUT_SUMMARY_DOUBLES; }
// criteria[8]: every entry finite, the reserved ones 0
static int rollout_check_criteria(const char* fn, const double* criteria) {
    for (int i = 0; i < SRBM_ROLLOUT_CRITERIA_DOUBLES; i++) {
        if (!std::isfinite(criteria[i])) return fail(std::string(fn) + ": criterion " + std::to_string(i) + " is not finite");
        if (i >= 6 && criteria[i] != 0.0) return fail(std::string(fn) + ": criterion " + std::to_string(i) + " is reserved and must be 0");
    }
    return 0;
}
static int rollout_enabled(const srbm_batch* h, const char* fn) {
    if (!h) return fail(std::string(fn) + ": bad arguments");
    if (!h->d_sum) return fail(std::string(fn) + ": no rollout summary is enabled on this batch (srbm_rollout_summary_enable)");
    return 0;
}
int srbm_rollout_summary_reset(srbm_batch* h) {
    if (rollout_enabled(h, "srbm_rollout_summary_reset")) return -1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_sum, h->sum_init.data(), sizeof(double) * h->sum_init.size(), hipMemcpyHostToDevice, h->stream));
    return 0;
}
int srbm_rollout_summary_enable(srbm_batch* h, const double* criteria, const double* ref) {
    if (!h) return fail("srbm_rollout_summary_enable: bad arguments");
    if (criteria) {
        if (!ref) return fail("srbm_rollout_summary_enable: criteria without references (ref[batch][6])");
        if (rollout_check_criteria("srbm_rollout_summary_enable", criteria)) return -1;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_sum) HIPCHK(hipFree(h->d_sum));
    h->d_sum = nullptr;
    if (h->d_sum_ref) HIPCHK(hipFree(h->d_sum_ref));
    h->d_sum_ref = nullptr;
    if (!criteria) return 0;
    const size_t B = h->batch;
    std::memcpy(h->sum_crit.c, criteria, sizeof(h->sum_crit.c));
    h->sum_init.resize(B * SRBM_ROLLOUT_SUMMARY_DOUBLES);
    for (size_t b = 0; b < B; b++) srbm_rollout_summary_init(h->sum_init.data() + b * SRBM_ROLLOUT_SUMMARY_DOUBLES);
    HIPCHK(hipMalloc(&h->d_sum_ref, sizeof(double) * SRBM_ROLLOUT_REF_DOUBLES * B));
    HIPCHK(hipMemcpy(h->d_sum_ref, ref, sizeof(double) * SRBM_ROLLOUT_REF_DOUBLES * B, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&h->d_sum, sizeof(double) * SRBM_ROLLOUT_SUMMARY_DOUBLES * B));
    return srbm_rollout_summary_reset(h);
}
int srbm_rollout_summary_fold(srbm_batch* h, int first_slot, int count) {
    if (!h) return fail("srbm_rollout_summary_fold: bad arguments");
    if (!h->d_log) return fail("srbm_rollout_summary_fold: no step log is enabled on this batch (srbm_step_log_enable)");
    if (rollout_enabled(h, "srbm_rollout_summary_fold")) return -1;
    if (first_slot < 0 || count < 0 || first_slot > h->log_used || count > h->log_used - first_slot)
        return fail("srbm_rollout_summary_fold: slots [" + std::to_string(first_slot) + ", " + std::to_string((long long)first_slot + count) + ") are outside the " +
                    std::to_string(h->log_used) + " steps logged");
    if (count == 0) return 0;
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_rollout_fold, dim3(h->batch), dim3(64), 0, h->stream, h->dp, h->d_log, h->batch, first_slot, count, h->sum_crit, h->d_sum_ref,
                       h->d_sum);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_rollout_summary_get(srbm_batch* h, int first, int count, double* out) {
    if (rollout_enabled(h, "srbm_rollout_summary_get")) return -1;
    if (!out) return fail("srbm_rollout_summary_get: bad arguments");
    if (first < 0 || count < 0 || first > h->batch || count > h->batch - first)
        return fail("srbm_rollout_summary_get: instances [" + std::to_string(first) + ", " + std::to_string((long long)first + count) + ") are outside the batch of " +
                    std::to_string(h->batch));
    if (count == 0) return 0;
    return fetch(h, {{out, h->d_sum + (size_t)first * SRBM_ROLLOUT_SUMMARY_DOUBLES, sizeof(double) * SRBM_ROLLOUT_SUMMARY_DOUBLES * count}});
}
int srbm_rollout_summary_copy_dev(srbm_batch* h, double* out_dev) {
    if (rollout_enabled(h, "srbm_rollout_summary_copy_dev")) return -1;
    if (!out_dev) return fail("srbm_rollout_summary_copy_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out_dev, h->d_sum, sizeof(double) * SRBM_ROLLOUT_SUMMARY_DOUBLES * (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
int srbm_rollout_study_dev(srbm_batch* h, const double* summaries_dev, int instances, double* study_dev) {
    if (!h || !summaries_dev || !study_dev || instances < 0) return fail("srbm_rollout_study_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(srbm_k_rollout_study, dim3(1), dim3(64), 0, h->stream, summaries_dev, instances, study_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_rollout_study(srbm_batch* h, double* study) {
    if (rollout_enabled(h, "srbm_rollout_study")) return -1;
    if (!study) return fail("srbm_rollout_study: bad arguments");
    void* d = nullptr;
    if (batch_scratch(h, sizeof(double) * SRBM_ROLLOUT_STUDY_DOUBLES, &d)) return -1;
    if (srbm_rollout_study_dev(h, h->d_sum, h->batch, static_cast<double*>(d))) return -1;
    return fetch(h, {{study, d, sizeof(double) * SRBM_ROLLOUT_STUDY_DOUBLES}});
}
// the same fold and the same reduction on the host: no GPU, no batch
int srbm_rollout_fold_host(const double* log, int slots, int batch, int first_slot, int count, const double* criteria, const double* ref, const double* mu,
                           double* summaries) {
    if (!log || !criteria || !ref || !mu || !summaries || slots < 0 || batch < 1) return fail("srbm_rollout_fold_host: bad arguments");
    if (rollout_check_criteria("srbm_rollout_fold_host", criteria)) return -1;
    if (first_slot < 0 || count < 0 || first_slot > slots || count > slots - first_slot)
        return fail("srbm_rollout_fold_host: slots [" + std::to_string(first_slot) + ", " + std::to_string((long long)first_slot + count) + ") are outside the " +
                    std::to_string(slots) + " slots of the log");
    for (int b = 0; b < batch; b++)
        for (int s = first_slot; s < first_slot + count; s++)
            srbm_rollout_fold_record(summaries + (size_t)b * SRBM_ROLLOUT_SUMMARY_DOUBLES, log + ((size_t)s * batch + b) * SRBM_STEP_LOG_DOUBLES, criteria,
                                     ref + (size_t)b * SRBM_ROLLOUT_REF_DOUBLES, mu[b]);
    return 0;
}
int srbm_rollout_study_host(const double* summaries, int instances, double* study) {
    if (!summaries || !study || instances < 0) return fail("srbm_rollout_study_host: bad arguments");
    double T[SRBM_ROLLOUT_STUDY_DOUBLES];
    srbm_rollout_study_init(T);
    for (int i = 0; i < instances; i++) srbm_rollout_study_add(T, summaries + (size_t)i * SRBM_ROLLOUT_SUMMARY_DOUBLES);
    std::memcpy(study, T, sizeof(T));
    return 0;
}
int srbm_synchronize(srbm_batch* h) {
    if (!h) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
void* srbm_stream(srbm_batch* h) { return h ? (void*)h->stream : nullptr; }

int srbm_update_contact_times(srbm_batch* h, const double* times, int max_contacts) {
    if (!h || !times || max_contacts <= 0) return fail("bad arguments");
    // the reference indexes the caller's vector with its own contact count (end_effector_splines.cpp:860-892): a vector that is
    // too short is an out-of-range read there, an error here
    std::string why;
    if (each_inst(h, [&](int b, const SrbmInst& I) {
            for (int ee = 0; ee < SRBM_NEE && why.empty(); ee++) {
                int n = 0;
                for (int i = 0; i < I.nk[ee]; i++) n += (I.kind[ee][i] <= SRBM_K_TD);
                if (n > max_contacts)
                    why = "srbm_update_contact_times: instance " + std::to_string(b) + " foot " + std::to_string(ee) + " has " + std::to_string(n) +
                          " contact times, max_contacts is " + std::to_string(max_contacts);
            }
        })) return -1;
    if (!why.empty()) return fail(why);
    void* d = nullptr;
    const size_t bytes = sizeof(double) * (size_t)h->batch * SRBM_NEE * max_contacts;
    if (batch_scratch(h, bytes, &d)) return -1;
    HIPCHK(hipMemcpyAsync(d, times, bytes, hipMemcpyHostToDevice, h->stream));
    if (upload_params(h)) return -1;
    const int tot = h->batch * SRBM_NEE;
    hipLaunchKernelGGL(srbm_k_set_contact_times, dim3((tot + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, static_cast<const double*>(d), max_contacts);
    HIPCHK(hipGetLastError());
    return srbm_synchronize(h);
}

// A solve that kernel 1 refused for capacity (SRBM_ERR_CAPACITY, status Other) assembled no QP: the sizes in the instance record and the counts in
// the work record are those of the schedule that did NOT fit, and nothing may be expanded or indexed by them (the debug exports refuse).
static bool refused_for_capacity(const SrbmInst& I) { return (I.err & SRBM_ERR_CAPACITY) != 0 && I.status == SRBM_OTHER; }
static std::string refused_message(const char* fn, int inst) {
    return std::string(fn) + ": the last solve of instance " + std::to_string(inst) + " was refused for capacity (SRBM_ERR_CAPACITY, status 8): "
           "no QP was assembled, its sizes belong to a schedule the build does not hold";
}

// ---------------- bilevel (gait) step: mpc::GaitOptimizer for the batch ----------------
struct srbm_gait {
    srbm_batch* h = nullptr;        // the instances being optimised
    srbm_batch* ls = nullptr;       // LS_SIZE candidates per instance, same stream
    double *xk = nullptr, *step = nullptr, *costs = nullptr, *dHdth = nullptr;   // [B][SRBM_GAIT_NV], costs [B][LS_SIZE]
    int *counts = nullptr, *imin = nullptr, *valid = nullptr, *lp_status = nullptr;   // [B][4], [B], [B], [B]
    double* pred_red = nullptr;                                                   // [B]
    int* ready = nullptr;                                                         // [B] deriv_ready of the controller
    SrbmGaitWork* gw = nullptr;                                                   // sensitivity workspace, one per instance
    unsigned ls_gen = 0;                                                          // params_gen of h the candidates' records were derived from
    bool times_read = false;        // xk / counts hold contact times read from a trajectory (srbm_gait_set_contact_times_from_trajectory ran since creation)
};

// the parameters of the candidate batch: candidate w = b * LS_SIZE + c solves with instance b's record
static void candidate_params(const srbm_batch* h, srbm_batch* c) {
    c->hp = h->hp; c->hp.batch = c->batch;
    c->im.resize(c->batch);
    for (int w = 0; w < c->batch; w++) c->im[w] = h->im[w / SRBM_LS_SIZE];
    c->params_dirty = true;
}

static int make_candidate_batch(const srbm_batch* h, srbm_batch** out) {
    auto* c = new srbm_batch;
    c->batch = h->batch * SRBM_LS_SIZE; c->device = h->device;
    candidate_params(h, c);
    if (alloc_batch(c, h->stream) || hipMemsetAsync(c->works, 0, sizeof(SrbmWork) * (size_t)c->batch, c->stream) != hipSuccess) {
        free_batch(c);
        return g_err.empty() ? fail("candidate batch: allocation failed") : -1;
    }
    *out = c;
    return 0;
}
static void free_gait(srbm_gait* g) {
    if (!g) return;
    (void)hipSetDevice(g->h->device);
    (void)hipStreamSynchronize(g->h->stream);
    if (g->ls) free_batch(g->ls);                    // (borrows the batch's stream: released before the batch, enforced by gait_refs)
    (void)hipFree(g->xk); (void)hipFree(g->step); (void)hipFree(g->dHdth); (void)hipFree(g->costs);
    (void)hipFree(g->counts); (void)hipFree(g->imin); (void)hipFree(g->gw); (void)hipFree(g->valid); (void)hipFree(g->lp_status);
    (void)hipFree(g->pred_red); (void)hipFree(g->ready);
    g->h->gait_refs--;
    delete g;
}
static int alloc_gait(srbm_gait* g) {
    srbm_batch* h = g->h;
    if (make_candidate_batch(h, &g->ls)) return -1;
    g->ls_gen = h->params_gen;
    const size_t B = h->batch;
    HIPCHK(hipMalloc(&g->xk, sizeof(double) * SRBM_GAIT_NV * B));
    HIPCHK(hipMalloc(&g->step, sizeof(double) * SRBM_GAIT_NV * B));
    HIPCHK(hipMalloc(&g->dHdth, sizeof(double) * SRBM_GAIT_NV * B));
    HIPCHK(hipMalloc(&g->costs, sizeof(double) * SRBM_LS_SIZE * B));
    HIPCHK(hipMalloc(&g->counts, sizeof(int) * SRBM_NEE * B));
    HIPCHK(hipMalloc(&g->imin, sizeof(int) * B));
    HIPCHK(hipMalloc(&g->valid, sizeof(int) * B));
    HIPCHK(hipMalloc(&g->lp_status, sizeof(int) * B));
    HIPCHK(hipMalloc(&g->pred_red, sizeof(double) * B));
    HIPCHK(hipMalloc(&g->ready, sizeof(int) * B));
    HIPCHK(hipMalloc(&g->gw, sizeof(SrbmGaitWork) * B));
    HIPCHK(hipMemsetAsync(g->ready, 0, sizeof(int) * B, h->stream));
    HIPCHK(hipMemsetAsync(g->lp_status, 0, sizeof(int) * B, h->stream));
    HIPCHK(hipMemsetAsync(g->pred_red, 0, sizeof(double) * B, h->stream));
    HIPCHK(hipMemsetAsync(g->valid, 0, sizeof(int) * B, h->stream));
    HIPCHK(hipMemsetAsync(g->counts, 0, sizeof(int) * SRBM_NEE * B, h->stream));
    HIPCHK(hipMemsetAsync(g->gw, 0, sizeof(SrbmGaitWork) * B, h->stream));
    HIPCHK(hipMemsetAsync(g->xk, 0, sizeof(double) * SRBM_GAIT_NV * B, h->stream));
    HIPCHK(hipMemsetAsync(g->step, 0, sizeof(double) * SRBM_GAIT_NV * B, h->stream));
    HIPCHK(hipMemsetAsync(g->dHdth, 0, sizeof(double) * SRBM_GAIT_NV * B, h->stream));
    return srbm_synchronize(h);
}

int srbm_gait_create(srbm_batch* h, srbm_gait** out) {
    if (!h || !out) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    auto* g = new srbm_gait;
    g->h = h;
    h->gait_refs++;
    if (alloc_gait(g)) { free_gait(g); return -1; }
    *out = g;
    return 0;
}
int srbm_gait_destroy(srbm_gait* g) {
    free_gait(g);
    return 0;
}
// GaitOptimizer::SetContactTimes(mpc.GetTrajectory().GetContactTimes()) (gait_optimizer.cpp:395-408)
int srbm_gait_set_contact_times_from_trajectory(srbm_gait* g) {
    if (!g) return fail("bad arguments");
    srbm_batch* h = g->h;
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_gait_read_contact_times, dim3((h->batch + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, g->xk, g->counts);
    HIPCHK(hipGetLastError());
    g->times_read = true;
    return 0;
}
int srbm_gait_get_contact_times(srbm_gait* g, double* xk, int* counts) {
    if (!g || !xk || !counts) return fail("bad arguments");
    const size_t B = g->h->batch;
    return fetch(g->h, {{xk, g->xk, sizeof(double) * SRBM_GAIT_NV * B}, {counts, g->counts, sizeof(int) * SRBM_NEE * B}});
}
int srbm_gait_set_step(srbm_gait* g, const double* step) {
    if (!g || !step) return fail("bad arguments");
    HIPCHK(hipSetDevice(g->h->device));
    HIPCHK(hipMemcpyAsync(g->step, step, sizeof(double) * SRBM_GAIT_NV * (size_t)g->h->batch, hipMemcpyHostToDevice, g->h->stream));
    return srbm_synchronize(g->h);
}
int srbm_gait_get_step(srbm_gait* g, double* step) {
    if (!g || !step) return fail("bad arguments");
    return fetch(g->h, {{step, g->step, sizeof(double) * SRBM_GAIT_NV * (size_t)g->h->batch}});
}
// MPC::ComputeDerivativeTerms (mpc.cpp:1047-1069): KKT sensitivity d = [dz; dlam; dnu] of the last QP solution
int srbm_gait_compute_sensitivity(srbm_gait* g) {
    if (!g) return fail("bad arguments");
    srbm_batch* h = g->h;
    if (h->last_tol_step > 0.0)
        return fail("srbm_gait_compute_sensitivity: the last solve of this batch ran with the step rule (tol_step > 0): its multipliers are not at the "
                    "gap tolerance the KKT sensitivity needs -- call srbm_set_solver_step_rule(h, 0, start_mu) before the solve that is differentiated "
                    "(srbm_gait_rti_advance does so by itself)");
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k3_normal_matrix, dim3(h->batch), dim3(K3_THREADS), K3_LDS_LAUNCH_BYTES, h->stream, h->dp, h->insts, h->works);
    hipLaunchKernelGGL(srbm_k_gait_sensitivity, dim3(h->batch), dim3(KG_THREADS), KG_DYN_LDS_BYTES, h->stream, h->dp, h->insts, h->works, g->gw);
    HIPCHK(hipGetLastError());
    return 0;
}
// mpc_controller.cpp:518-561: SetContactTimes, ComputeDerivativeTerms / GetQPPartials, the 20 parameter partials and
// GaitOptimizer::ComputeCostFcnDerivWrtContactTimes, for every instance.  dHdth stays on the device for the LP.
int srbm_gait_compute_gradient(srbm_gait* g) {
    if (!g) return fail("bad arguments");
    srbm_batch* h = g->h;
    if (srbm_gait_set_contact_times_from_trajectory(g)) return -1;
    if (srbm_gait_compute_sensitivity(g)) return -1;
    hipLaunchKernelGGL(srbm_k_gait_gradient, dim3(h->batch), dim3(KH_THREADS), 0, h->stream, h->dp, h->insts, h->works, g->gw, g->dHdth, g->valid);
    HIPCHK(hipGetLastError());
    return 0;
}
// MPCSingleRigidBody::ComputeParamPartialsClarabel (msrb.cpp:642-792) as data: the partials of the QP of the LAST solve of instance `inst` with
// respect to contact time `idx` of foot `ee`, evaluated on the instance's current trajectory, dense and in the reference's layout
// (mpc::QPPartials, mpc/include/qp/qp_partials.h:15-35): dA [n_eq][n], dG [n_ineq][n], db [n_eq], dh [n_ineq] (zero as coded).  Debug path like
// srbm_export_qp: it runs the SAME per-item code the gradient kernel contracts (gait_param_partial_item), with a dense emitter.
int srbm_gait_get_param_partials(srbm_batch* h, int inst, int ee, int idx, double* dA, double* dG, double* db, double* dh) {
    if (!h || inst < 0 || inst >= h->batch || ee < 0 || ee >= SRBM_NEE || idx < 0 || !dA || !dG || !db || !dh) return fail("bad arguments");
    if (use_batch(h)) return -1;
    SrbmInst I;
    if (fetch(h, {{&I, h->insts + inst, sizeof(SrbmInst)}})) return -1;
    if (refused_for_capacity(I)) return fail(refused_message("srbm_gait_get_param_partials", inst));
    const size_t n = I.n, me = I.n_eq, mi = I.n_ineq;
    if (n == 0 || me == 0) return fail("srbm_gait_get_param_partials: no QP has been solved yet");
    double* d = nullptr;
    const size_t tot = me * n + mi * n + me + 1;
    DevTemps tmp;
    HIPCHK(tmp.alloc(&d, sizeof(double) * tot));
    HIPCHK(hipMemsetAsync(d, 0, sizeof(double) * tot, h->stream));
    int* derr = reinterpret_cast<int*>(d + me * n + mi * n + me);
    hipLaunchKernelGGL(srbm_k_gait_param_partials, dim3(1), dim3(KH_THREADS), 0, h->stream, h->dp + inst, h->insts + inst, h->works + inst, ee, idx,
                       d, d + me * n, d + me * n + mi * n, derr);
    HIPCHK(hipGetLastError());
    int err = 0;
    if (fetch(h, {{dA, d, sizeof(double) * me * n}, {dG, d + me * n, sizeof(double) * mi * n}, {db, d + me * n + mi * n, sizeof(double) * me},
                  {&err, derr, sizeof(int)}})) return -1;
    std::memset(dh, 0, sizeof(double) * mi);
    if (err & SRBM_ERR_CAPACITY) return fail("srbm_gait_get_param_partials: contact index out of range");
    if (err) return fail("srbm_gait_get_param_partials: spline lookup failed (error bits " + std::to_string(err) + ")");
    return 0;
}
int srbm_gait_get_gradient(srbm_gait* g, double* dHdth, int* valid) {
    if (!g || !dHdth) return fail("bad arguments");
    const size_t B = g->h->batch;
    return fetch(g->h, {{dHdth, g->dHdth, sizeof(double) * SRBM_GAIT_NV * B}, {valid, g->valid, sizeof(int) * B}});
}
int srbm_gait_set_gradient(srbm_gait* g, const double* dHdth, const int* valid) {
    if (!g || !dHdth || !valid) return fail("bad arguments");
    const size_t B = g->h->batch;
    HIPCHK(hipSetDevice(g->h->device));
    HIPCHK(hipMemcpyAsync(g->dHdth, dHdth, sizeof(double) * SRBM_GAIT_NV * B, hipMemcpyHostToDevice, g->h->stream));
    HIPCHK(hipMemcpyAsync(g->valid, valid, sizeof(int) * B, hipMemcpyHostToDevice, g->h->stream));
    return srbm_synchronize(g->h);
}
int srbm_gait_get_sensitivity(srbm_gait* g, double* d, int ld) {
    if (!g || !d || ld <= 0) return fail("bad arguments");
    srbm_batch* h = g->h;
    HIPCHK(hipSetDevice(h->device));
    void* devv = nullptr;
    const size_t bytes = sizeof(double) * (size_t)h->batch * ld;
    if (batch_scratch(h, bytes, &devv)) return -1;
    double* dev = static_cast<double*>(devv);
    HIPCHK(hipMemsetAsync(dev, 0, bytes, h->stream));
    hipLaunchKernelGGL(srbm_k_gait_pack_d, dim3(h->batch), dim3(128), 0, h->stream, h->dp, h->insts, h->works, g->gw, dev, ld);
    HIPCHK(hipGetLastError());
    return fetch(h, {{d, dev, bytes}});
}
// the LP of the gait step on the gradient dHdth and the time in h->d_time (srbm_gait.hiph)
static void launch_gait_lp(srbm_gait* g) {
    srbm_batch* h = g->h;
    hipLaunchKernelGGL(srbm_k_gait_lp, dim3(h->batch), dim3(LP_THREADS), 0, h->stream, h->dp, h->insts, g->xk, g->counts, g->dHdth, h->d_time,
                       g->step, g->pred_red, g->lp_status);
}
// deriv_ready of every instance: `force` (0 / 1), or -1 for "a gradient exists and its LP was solved"
static void launch_gait_ready(srbm_gait* g, int force) {
    srbm_batch* h = g->h;
    hipLaunchKernelGGL(srbm_k_gait_ready, dim3((h->batch + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, g->valid, g->lp_status, g->ready, force);
}
// GaitOptimizer::OptimizeContactTimes (gait_optimizer.cpp:185-364): the LP over the contact-time step; time[batch]
int srbm_gait_optimize_contact_times(srbm_gait* g, const double* time) {
    if (!g || !time) return fail("bad arguments");
    srbm_batch* h = g->h;
    if (use_batch(h)) return -1;
    HIPCHK(hipMemcpyAsync(h->d_time, time, sizeof(double) * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    launch_gait_lp(g);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_gait_get_lp_result(srbm_gait* g, int* lp_status, double* pred_red) {
    if (!g) return fail("bad arguments");
    const size_t B = g->h->batch;
    return fetch(g->h, {{lp_status, g->lp_status, sizeof(int) * B}, {pred_red, g->pred_red, sizeof(double) * B}});
}
// the records of the batch and of its candidates on the device as the host has them
static int candidate_records_current(srbm_gait* g) {
    srbm_batch* h = g->h; srbm_batch* ls = g->ls;
    if (upload_params(h)) return -1;
    if (g->ls_gen != h->params_gen) { candidate_params(h, ls); g->ls_gen = h->params_gen; }     // costs / tolerances changed since the last line search
    return upload_params(ls);
}
// candidates -> 10*B solves -> argmin + install; inputs already in h->d_state / d_time / d_ee
static int line_search_core(srbm_gait* g, bool use_ready_mask) {
    srbm_batch* h = g->h; srbm_batch* ls = g->ls;
    const int B = h->batch;
    if (candidate_records_current(g)) return -1;
    const int* ready = use_ready_mask ? g->ready : nullptr;
    hipLaunchKernelGGL(srbm_k_gait_spawn_candidates, dim3(B * SRBM_LS_SIZE), dim3(128), 0, h->stream, h->dp, h->insts, ls->insts,
                       g->xk, g->step, h->d_state, h->d_time, h->d_ee, ls->d_state, ls->d_time, ls->d_ee, ready);
    HIPCHK(hipGetLastError());
    if (launch_step(ls)) return -1;
    hipLaunchKernelGGL(srbm_k_gait_select, dim3(B), dim3(128), 0, h->stream, h->dp, h->insts, ls->insts, h->works, ls->works, ready, g->imin, g->costs);
    HIPCHK(hipGetLastError());
    return 0;
}
// GaitOptimizer::LineSearch (gait_optimizer.cpp:671-753)
int srbm_gait_line_search(srbm_gait* g, const double* state, const double* time, const double* ee, int* imin, double* costs) {
    if (!g || !state || !time || !ee) return fail("bad arguments");
    srbm_batch* h = g->h;
    // every candidate's schedule is x_k + (i/10) step: with x_k never read, the zeros of the allocation (no ready mask here to keep the schedules)
    if (!g->times_read)
        return fail("srbm_gait_line_search: this handle has not read any contact times since it was created -- call "
                    "srbm_gait_set_contact_times_from_trajectory (or srbm_gait_compute_gradient, which does) first");
    HIPCHK(hipSetDevice(h->device));
    if (upload_inputs(h, state, time, ee)) return -1;
    if (line_search_core(g, false)) return -1;
    const size_t B = h->batch;
    return fetch(h, {{imin, g->imin, sizeof(int) * B}, {costs, g->costs, sizeof(double) * SRBM_LS_SIZE * B}});
}
// MPCController::GaitOpt (mpc_controller.cpp:518-566): gradient + LP at `time`; sets deriv_ready per instance
static int gait_opt_core(srbm_gait* g) {        // time already in h->d_time
    if (srbm_gait_compute_gradient(g)) return -1;
    launch_gait_lp(g);
    launch_gait_ready(g, -1);
    HIPCHK(hipGetLastError());
    return 0;
}
// The MPC loop of the controller with the bilevel step folded in (mpc_controller.cpp:320-346), device-resident and
// open-loop as srbm_rti_advance (state := node 1 of the previous trajectory, time = run_num * dt):
//   run_num % freq == 0 and a gradient is ready  -> LineSearch only (its 10 candidates are the RTI solves of this step)
//   (run_num + 1) % freq == 0                     -> GetRealTimeUpdate, then GaitOpt (gradient + LP for the next step)
//   otherwise                                     -> GetRealTimeUpdate
int srbm_gait_rti_advance(srbm_gait* g, int first_run_num, int steps, int gait_opt_freq) {
    if (!g || steps < 0 || gait_opt_freq <= 0) return fail("bad arguments");
    srbm_batch* h = g->h;
    if (use_batch(h)) return -1;
    for (int i = 0; i < steps; i++) {
        const int run_num = first_run_num + i;
        const double time = run_num * h->hp.dt;
        hipLaunchKernelGGL(srbm_k_next_inputs, dim3(h->batch), dim3(64), 0, h->stream, h->dp, h->insts, time, h->d_state, h->d_time, h->d_ee);
        if (run_num % gait_opt_freq == 0 && run_num > 0) {
            // instances without a ready gradient get the plain update through the same 10-candidate batch (zero step)
            if (line_search_core(g, true)) return -1;
            launch_gait_ready(g, 0);
        } else if ((run_num + 1) % gait_opt_freq == 0 && run_num > 0) {
            // the solve the gradient differentiates: to the reference's gap criterion (the as-coded KKT sensitivity divides by the slacks, so it
            // needs the duals Clarabel's tolerance gives); every other solve of the protocol -- plain steps, the 10 candidates of a line
            // search, which are only compared by cost -- runs with the batch's step rule
            if (launch_step(h, true)) return -1;
            if (gait_opt_core(g)) return -1;
        } else {
            if (launch_step(h)) return -1;
            launch_gait_ready(g, 0);
        }
        HIPCHK(hipGetLastError());
    }
    return 0;
}
// ---- closed-loop rollout with the gait step (include/srbm_rti.h; srbm_gait_rollout.hiph) ----
// the plant half of closed-loop iteration `index` on its own kernel: h->d_plant advanced, h->d_state / d_time / d_ee filled
static int launch_plant(srbm_batch* h, int index, int substeps, int advance_time) {
    const SrbmPlantArgs pl = plant_args(h, substeps, advance_time);
    hipLaunchKernelGGL(srbm_k_plant_inputs, dim3(h->batch), dim3(GR_PLANT_THREADS), 0, h->stream, h->dp, h->insts, index, pl.period, pl.substeps, pl.advance_time,
                       pl.plant, pl.push, h->d_state, h->d_time, h->d_ee);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_plant_advance(srbm_batch* h, int index, int substeps, int advance_time, double* state, double* time, double* ee) {
    if (!h || substeps < 1) return fail("srbm_plant_advance: bad arguments");
    if (!h->d_plant) return fail("srbm_plant_advance: the plant state has not been set (srbm_plant_set_state)");
    if (use_batch(h) || launch_plant(h, index, substeps, advance_time)) return -1;
    const size_t B = h->batch;
    return fetch(h, {{state, h->d_state, sizeof(double) * 13 * B}, {time, h->d_time, sizeof(double) * B}, {ee, h->d_ee, sizeof(double) * 12 * B}});
}
// the record of the gradient or line-search run just queued (srbm_k_gait_step_log)
static int log_gait_step(srbm_gait* g, int run) {
    srbm_batch* h = g->h;
    if (!h->d_log) return 0;
    hipLaunchKernelGGL(srbm_k_gait_step_log, dim3(h->batch), dim3(64), 0, h->stream, h->insts, h->d_state, h->d_time, h->d_ee, log_args(h), run, g->ready,
                       g->lp_status, g->pred_red, g->imin, g->costs);
    HIPCHK(hipGetLastError());
    h->log_used++;
    return 0;
}
// The controller loop of srbm_gait_rti_advance closed over the plant of srbm_closed_loop_advance: run r integrates the plant from (r - 1) p to r p,
// p the MPC period of the instance (iteration r - 1 of srbm_closed_loop_advance) and branches on r as srbm_gait_rti_advance does.  A maximal stretch of plain runs is ONE multi-step plant
// launch (launch_fused: the step queues for a batch larger than the chip); gradient and line-search runs take the plant kernel, then the one-step kernels.
int srbm_gait_closed_loop_advance(srbm_gait* g, int first_run_num, int steps, int gait_opt_freq, int substeps, int advance_time) {
    const char* fn = "srbm_gait_closed_loop_advance";
    if (!g) return fail(std::string(fn) + ": bad arguments (NULL handle)");
    srbm_batch* h = g->h;
    if (first_run_num < 1) return fail(std::string(fn) + ": first_run_num must be at least 1 (run r integrates the plant from (r - 1) dt to r dt)");
    if (steps < 0 || gait_opt_freq <= 0 || substeps < 1) return fail(std::string(fn) + ": bad arguments (steps >= 0, gait_opt_freq > 0, substeps >= 1)");
    if (!h->d_plant) return fail(std::string(fn) + ": the plant state has not been set (srbm_plant_set_state)");
    if (log_room(h, fn, steps)) return -1;
    if (use_batch(h)) return -1;
    const int F = gait_opt_freq, end = first_run_num + steps;
    auto plain = [F](int r) { return r % F != 0 && (r + 1) % F != 0; };
    for (int r = first_run_num; r < end;) {
        if (plain(r)) {
            int n = 1;
            while (r + n < end && plain(r + n)) n++;
            if (launch_fused(h, fn, r - 1, n, plant_args(h, substeps, advance_time))) return -1;
            launch_gait_ready(g, 0);
            r += n;
        } else if (r % F == 0) {
            // instances without a ready gradient get the plain update through the same 10-candidate batch (zero step)
            if (launch_plant(h, r - 1, substeps, advance_time) || line_search_core(g, true)) return -1;
            if (log_gait_step(g, SRBM_GAIT_RUN_LINE_SEARCH)) return -1;          // before the flag is reset: it tells who searched
            launch_gait_ready(g, 0);
            r++;
        } else {
            // the solve the gradient differentiates: to the gap criterion whatever the batch's step rule says (srbm_gait_rti_advance)
            if (launch_plant(h, r - 1, substeps, advance_time) || launch_step(h, true) || gait_opt_core(g)) return -1;
            if (log_gait_step(g, SRBM_GAIT_RUN_GRADIENT)) return -1;
            r++;
        }
        HIPCHK(hipGetLastError());
    }
    return 0;
}
int srbm_gait_get_line_search_result(srbm_gait* g, int* imin, double* costs) {
    if (!g) return fail("srbm_gait_get_line_search_result: bad arguments");
    const size_t B = g->h->batch;
    return fetch(g->h, {{imin, g->imin, sizeof(int) * B}, {costs, g->costs, sizeof(double) * SRBM_LS_SIZE * B}});
}
// diagnostic / test hook: the batch of line-search candidates (LS_SIZE per instance, candidate c of instance b at index b * LS_SIZE + c), owned by
// the gait handle -- for the read-back entries (status, sizes, srbm_export_qp) only
srbm_batch* srbm_gait_debug_candidates(srbm_gait* g) { return g ? g->ls : nullptr; }
// status and error bits of the candidates of the last line search: status[batch * LS_SIZE], err[batch * LS_SIZE] (diagnostic)
int srbm_gait_get_candidate_status(srbm_gait* g, int* status, int* err) {
    if (!g || !status || !err) return fail("bad arguments");
    return each_inst(g->ls, [&](int b, const SrbmInst& I) { status[b] = I.status; err[b] = I.err | I.err_acc; });
}

// MPC::AdjustForCurrentContacts (mpc.cpp:1195-1203): time[batch], in_contact[batch][4]
int srbm_adjust_for_current_contacts(srbm_batch* h, const double* time, const int* in_contact) {
    if (!h || !time || !in_contact) return fail("bad arguments");
    if (use_batch(h)) return -1;
    void* dcv = nullptr;
    const size_t B = h->batch;
    if (batch_scratch(h, sizeof(int) * 4 * B, &dcv)) return -1;
    int* dc = static_cast<int*>(dcv);
    HIPCHK(hipMemcpyAsync(dc, in_contact, sizeof(int) * 4 * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_time, time, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    const int tot = h->batch * SRBM_NEE;
    hipLaunchKernelGGL(srbm_k_adjust_for_current_contacts, dim3((tot + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, h->d_time, dc);
    HIPCHK(hipGetLastError());
    return srbm_synchronize(h);
}

int srbm_enable_kernel_timing(srbm_batch* h, int max_launches) {
    if (!h || max_launches < 0) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    while ((int)h->ev_start.size() < max_launches) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
        h->ev_start.push_back(a); h->ev_stop.push_back(b); h->ev_steps.push_back(0);
    }
    h->ev_used = 0; h->timing = max_launches > 0;
    return 0;
}
int srbm_get_kernel_timing(srbm_batch* h, double* total_ms, int* launches) {
    if (!h || !total_ms || !launches) return fail("bad arguments");
    if (srbm_synchronize(h)) return -1;
    double tot = 0;
    for (size_t i = 0; i < h->ev_used; i++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_start[i], h->ev_stop[i])); tot += ms; }
    *total_ms = tot; *launches = (int)h->ev_used;
    return 0;
}
int srbm_get_kernel_timings(srbm_batch* h, double* ms_each, int max_launches, int* launches) {
    if (!h || !ms_each || !launches || max_launches < 0) return fail("bad arguments");
    if (srbm_synchronize(h)) return -1;
    *launches = (int)h->ev_used;
    for (size_t i = 0; i < h->ev_used && (int)i < max_launches; i++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_start[i], h->ev_stop[i])); ms_each[i] = ms; }
    return 0;
}
// per instance: the running total of factorisations (diagnostic: scripts/dev_dispatch_order.py)
int srbm_debug_get_instance_iters(srbm_batch* h, double* iters /* [batch] */) {
    if (!h || !iters) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { iters[b] = I.acc_iters; });
}
// which kernel the last srbm_rti_advance / srbm_closed_loop_advance with steps > 0 took (tests/test_gpu_launch_equivalence.py):
// out4 = {CUs of the device, kernel (0 none yet, 1 srbm_rti_fused, 2 srbm_rti_fused_long, 3 srbm_rti_queued, 4 srbm_rti_queued_long), its steps,
// 1 if that launch ran on the step queues}.  Host-side record of the choice made at launch; reads no device memory.
int srbm_debug_get_launch_info(const srbm_batch* h, int* out4) {
    if (!h || !out4) return fail("bad arguments");
    out4[0] = h->n_cu; out4[1] = h->last_launch_kernel; out4[2] = h->last_launch_steps; out4[3] = h->last_launch_kernel >= 3 ? 1 : 0;
    return 0;
}
int srbm_get_work_counters(srbm_batch* h, double* total_ipm_iterations, double* total_algorithmic_flops) {
    if (!h) return fail("bad arguments");
    double it = 0, fl = 0;
    if (each_inst(h, [&](int, const SrbmInst& I) { it += I.acc_iters; fl += I.acc_flops; })) return -1;
    if (total_ipm_iterations) *total_ipm_iterations = it;
    if (total_algorithmic_flops) *total_algorithmic_flops = fl;
    return 0;
}
int srbm_pack_results_dev(srbm_batch* h, double* out_dev, int ld) {
    if (!h || !out_dev || ld < 8) return fail("bad arguments");
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_pack_results, dim3(h->batch), dim3(64), 0, h->stream, h->dp, h->insts, h->works, out_dev, ld);
    HIPCHK(hipGetLastError());
    return 0;
}

int srbm_pack_results(srbm_batch* h, double* out, int ld) {
    if (!h || !out || ld < 8) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    void* d = nullptr;
    const size_t bytes = sizeof(double) * (size_t)h->batch * ld;
    if (batch_scratch(h, bytes, &d)) return -1;
    if (srbm_pack_results_dev(h, static_cast<double*>(d), ld)) return -1;
    return fetch(h, {{out, d, bytes}});
}

// ---------------- multi-GPU: RCCL all-gather of the result records (include/srbm_rti.h) ----------------
// RCCL is bound at run time (types from its header, no link dependency): a process that has a copy loaded -- a C++ host linked against
// librccl.so.1, a Python process whose torch brought its own librccl.so -- gets THAT copy, so that a ncclComm_t made on the caller's side and the
// calls made here belong to the same library.
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
};
static RcclApi* rccl_api_ptr() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* forced = std::getenv("SRBM_RCCL_LIB");
        const char* names[] = {"librccl.so", "librccl.so.1"};
        if (forced) api.lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        for (int pass = 0; pass < 2 && !api.lib && !forced; pass++)                   // pass 0: a copy already in the process, pass 1: load one
            for (const char* n : names) if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
        if (!api.lib) { const char* e = dlerror(); api.err = std::string("RCCL not found (librccl.so / librccl.so.1; SRBM_RCCL_LIB overrides): ") + (e ? e : ""); return; }
        auto sym = [&](const char* n) { void* p = dlsym(api.lib, n); if (!p && api.err.empty()) api.err = std::string("RCCL symbol missing: ") + n; return p; };
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(sym("ncclCommUserRank"));
        api.CommCount = reinterpret_cast<decltype(api.CommCount)>(sym("ncclCommCount"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    });
    return &api;
}
#define rccl_api() (*rccl_api_ptr())
static int rccl_fail(const char* what, ncclResult_t r) {
    RcclApi& A = rccl_api();
    return fail(std::string(what) + ": " + (A.GetErrorString ? A.GetErrorString(r) : "RCCL error"));
}
static_assert(sizeof(ncclUniqueId) == SRBM_RCCL_UNIQUE_ID_BYTES, "include/srbm_rti.h states the size of ncclUniqueId");

int srbm_rccl_get_unique_id(void* id_bytes) {
    if (!id_bytes) return fail("bad arguments");
    RcclApi& A = rccl_api();
    if (!A.err.empty()) return fail(A.err);
    ncclUniqueId id;
    const ncclResult_t r = A.GetUniqueId(&id);
    if (r != ncclSuccess) return rccl_fail("ncclGetUniqueId", r);
    std::memcpy(id_bytes, &id, sizeof(id));
    return 0;
}
int srbm_rccl_comm_init_rank(srbm_batch* h, int world, int rank, const void* id_bytes, ncclComm_t* comm_out) {
    if (!h || !id_bytes || !comm_out || world < 1 || rank < 0 || rank >= world) return fail("bad arguments");
    RcclApi& A = rccl_api();
    if (!A.err.empty()) return fail(A.err);
    HIPCHK(hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id_bytes, sizeof(id));
    const ncclResult_t r = A.CommInitRank(comm_out, world, id, rank);
    if (r != ncclSuccess) return rccl_fail("ncclCommInitRank", r);
    return 0;
}
int srbm_rccl_comm_destroy(ncclComm_t comm) {
    if (!comm) return 0;
    RcclApi& A = rccl_api();
    if (!A.err.empty()) return fail(A.err);
    const ncclResult_t r = A.CommDestroy(comm);
    if (r != ncclSuccess) return rccl_fail("ncclCommDestroy", r);
    return 0;
}
// The two halves of an in-place all-gather of `count` doubles per rank on the batch's stream.  allgather_slot: RCCL bound, the communicator asked for
// rank and world, *mine = this rank's slot of out_dev (the caller queues its doubles straight into it); allgather_run: ONE ncclAllGather.
static int allgather_slot(const char* fn, srbm_batch* h, ncclComm_t comm, double* out_dev, size_t count, double** mine) {
    if (!h || !comm || !out_dev) return fail("bad arguments");
    RcclApi& A = rccl_api();
    if (!A.err.empty()) return fail(A.err);
    HIPCHK(hipSetDevice(h->device));
    int rank = -1, world = 0;
    ncclResult_t r = A.CommUserRank(comm, &rank);
    if (r == ncclSuccess) r = A.CommCount(comm, &world);
    if (r != ncclSuccess) return rccl_fail("ncclCommUserRank / ncclCommCount", r);
    if (rank < 0 || rank >= world) return fail(std::string(fn) + ": communicator reports an invalid rank");
    *mine = out_dev + (size_t)rank * count;
    return 0;
}
static int allgather_run(srbm_batch* h, ncclComm_t comm, double* mine, double* out_dev, size_t count) {
    const ncclResult_t r = rccl_api().AllGather(mine, out_dev, count, ncclDouble, comm, h->stream);
    if (r != ncclSuccess) return rccl_fail("ncclAllGather", r);
    return 0;
}
int srbm_allgather_results(srbm_batch* h, ncclComm_t comm, double* out_dev) {
    if (!h) return fail("bad arguments");
    const int ld = srbm_result_record_doubles(h->hp.N);
    const size_t count = (size_t)h->batch * ld;
    double* mine = nullptr;
    if (allgather_slot("srbm_allgather_results", h, comm, out_dev, count, &mine)) return -1;
    if (srbm_pack_results_dev(h, mine, ld)) return -1;
    return allgather_run(h, comm, mine, out_dev, count);
}
int srbm_rollout_allgather_dev(srbm_batch* h, ncclComm_t comm, double* out_dev) {
    if (rollout_enabled(h, "srbm_rollout_allgather_dev")) return -1;
    const size_t count = (size_t)h->batch * SRBM_ROLLOUT_SUMMARY_DOUBLES;
    double* mine = nullptr;
    if (allgather_slot("srbm_rollout_allgather_dev", h, comm, out_dev, count, &mine)) return -1;
    if (srbm_rollout_summary_copy_dev(h, mine)) return -1;
    return allgather_run(h, comm, mine, out_dev, count);
}

// ---------------- getters ----------------
int srbm_get_sizes(srbm_batch* h, int* sizes) {
    if (!h || !sizes) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) {
        int* s = sizes + 8 * b;
        s[0] = I.n; s[1] = I.m; s[2] = I.n_eq; s[3] = I.n_ineq; s[4] = I.nfv; s[5] = I.npv; s[6] = I.n_td; s[7] = I.n_samples;
    });
}
int srbm_get_status(srbm_batch* h, int* status, int* err) {
    if (!h || !status) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { status[b] = I.status; if (err) err[b] = I.err; });
}
// QP objective at the raw QP minimiser (the "QP Cost" column of MPC::PrintStatLineToFile, mpc.cpp:989): cost[batch]
int srbm_get_qp_cost(srbm_batch* h, double* cost) {
    if (!h || !cost) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { cost[b] = I.qp_cost; });
}
int srbm_get_stats(srbm_batch* h, double* stats) {
    if (!h || !stats) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) {
        double* s = stats + 8 * b;
        s[0] = I.alpha; s[1] = I.cost; s[2] = I.eq_violation; s[3] = I.step_norm; s[4] = I.qp_iters; s[5] = I.res_primal; s[6] = I.res_dual; s[7] = I.gap;
    });
}
int srbm_get_trajectory_states(srbm_batch* h, double* states) {
    if (!h || !states) return fail("bad arguments");
    const int len = (h->hp.N + 1) * 13;
    return each_inst(h, [&](int b, const SrbmInst& I) { std::memcpy(states + (size_t)b * len, I.states, sizeof(double) * len); });
}
int srbm_get_qp_solution(srbm_batch* h, double* x, int ld) {
    if (!h || !x) return fail("bad arguments");
    return fetch_work_field(h, offsetof(SrbmWork, x), std::min<size_t>(ld, SRBM_NXMAX), x, ld);
}
int srbm_get_raw_qp_minimiser(srbm_batch* h, double* x, int ld) {
    if (!h || !x) return fail("bad arguments");
    return fetch_work_field(h, offsetof(SrbmWork, x_qp), std::min<size_t>(ld, SRBM_NXMAX), x, ld);
}
int srbm_get_dual_solution(srbm_batch* h, double* z, double* s, int ld) {
    if (!h || !z) return fail("bad arguments");
    if (fetch_work_field(h, offsetof(SrbmWork, z), std::min<size_t>(ld, SRBM_MMAX), z, ld)) return -1;
    if (s) return fetch_work_field(h, offsetof(SrbmWork, s), std::min<size_t>(ld, SRBM_MMAX), s, ld);
    return 0;
}
int srbm_get_knots(srbm_batch* h, int inst, double* times, int* kinds, int* nk, double* fvals, double* pvals, double* box) {
    if (!h || inst < 0 || inst >= h->batch) return fail("bad arguments");
    std::vector<SrbmInst> v(1);
    if (fetch(h, {{v.data(), h->insts + inst, sizeof(SrbmInst)}})) return -1;
    const SrbmInst& I = v[0];
    for (int ee = 0; ee < SRBM_NEE; ee++) {
        if (nk) nk[ee] = I.nk[ee];
        for (int k = 0; k < SRBM_KMAX; k++) {
            if (times) times[ee * SRBM_KMAX + k] = I.knot_t[ee][k];
            if (kinds) kinds[ee * SRBM_KMAX + k] = I.kind[ee][k];
        }
    }
    if (fvals) std::memcpy(fvals, I.fval, sizeof(I.fval));
    if (pvals) std::memcpy(pvals, I.pval, sizeof(I.pval));
    if (box) { box[0] = I.box[0]; box[1] = I.box[1]; }
    return 0;
}

// Dense expansion of the structured QP into the reference's row/column layout.  Its dynamics rows are the host's
// statement of the model that csrc/srbm_lin.hiph holds for the device.
int srbm_export_qp(srbm_batch* h, int inst, double* A, double* b, double* Pm, double* q) {
    if (!h || inst < 0 || inst >= h->batch) return fail("bad arguments");
    std::vector<SrbmInst> vi(1);
    std::vector<SrbmWork> vw(1);
    if (fetch(h, {{vi.data(), h->insts + inst, sizeof(SrbmInst)}, {vw.data(), h->works + inst, sizeof(SrbmWork)}})) return -1;
    const SrbmInst& I = vi[0];
    const SrbmWork& W = vw[0];
    if (refused_for_capacity(I)) return fail(refused_message("srbm_export_qp", inst));
    SrbmParams P = inst_params(h, inst);
    if (h->d_cmd) {          // with a command schedule set the linear costs are the device's: what the last command wrote (srbm_command.hiph)
        if (use_batch(h)) return -1;
        const char* const rec = reinterpret_cast<const char*>(h->dp + inst);
        if (fetch(h, {{P.w, rec + offsetof(SrbmParams, w), sizeof(P.w)}, {P.Phi_w, rec + offsetof(SrbmParams, Phi_w), sizeof(P.Phi_w)}})) return -1;
    }
    const int N = P.N, n = I.n, m = I.m, nx = (N + 1) * 12, ns = W.n_samp;
    const double dt = P.dt;
    if (A) std::memset(A, 0, sizeof(double) * (size_t)m * n);
    if (b) std::memset(b, 0, sizeof(double) * m);
    if (Pm) std::memset(Pm, 0, sizeof(double) * (size_t)n * n);
    if (q) std::memset(q, 0, sizeof(double) * n);
    auto Aat = [&](int r, int c) -> double& { return A[(size_t)r * n + c]; };
    if (A && b) {
        // dynamics rows (msrb.cpp:218-265)
        for (int i = 0; i < 12; i++) { Aat(i, i) = -1; b[i] = -W.xbar[i]; }
        for (int k = 0; k < N; k++) {
            const int r0 = 12 * (k + 1);
            for (int i = 0; i < 12; i++) { Aat(r0 + i, 12 * k + i) += 1.0; Aat(r0 + i, 12 * (k + 1) + i) += -1.0; b[r0 + i] = -W.craw[k][i]; }
            for (int i = 0; i < 3; i++) Aat(r0 + i, 12 * k + 3 + i) += dt * (1.0 / P.mass);
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
                Aat(r0 + 6 + i, 12 * k + 9 + j) += dt * P.Ir_inv[3 * i + j];
                Aat(r0 + 9 + i, 12 * k + j) += dt * W.ALp[k][3 * i + j];
                Aat(r0 + 9 + i, 12 * k + 9 + j) += dt * W.ALL[k][3 * i + j];
            }
            for (int ee = 0; ee < SRBM_NEE; ee++) {
                const SrbmNodeRec& r = W.node[k][ee];
                const double d[3] = {r.r[0] - W.xbar[12 * k], r.r[1] - W.xbar[12 * k + 1], r.r[2] - W.xbar[12 * k + 2]};
                for (int c = 0; c < 3; c++) {
                    double e[3] = {0, 0, 0}; e[c] = 1;
                    const double dxe[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
                    if (r.fmut) for (int p = 0; p < r.fcnt; p++) {
                        const int col = nx + W.fbase[ee][c] + r.fidx + p;
                        Aat(r0 + 3 + c, col) = dt * r.flin[p];
                        for (int qd = 0; qd < 3; qd++) Aat(r0 + 9 + qd, col) = dt * (dxe[qd] * r.flin[p]);
                    }
                    if (c < 2) {
                        const double exf[3] = {e[1] * r.f[2] - e[2] * r.f[1], e[2] * r.f[0] - e[0] * r.f[2], e[0] * r.f[1] - e[1] * r.f[0]};
                        for (int p = 0; p < r.pcnt; p++) {
                            const int col = nx + W.pbase[ee][c] + r.pidx + p;
                            for (int qd = 0; qd < 3; qd++) Aat(r0 + 9 + qd, col) = dt * (exf[qd] * r.plin[p]);
                        }
                    }
                }
            }
        }
        // force box + friction pyramid (mpc.cpp:352-414, 166-208; qp_data.cpp:256)
        int row = nx;
        for (int j = 0; j < 2; j++)
            for (int s = 0; s < ns; s++) {
                const SrbmSample& sm = W.samp[s];
                for (int p = 0; p < sm.cnt; p++) Aat(row, nx + W.fbase[sm.ee][2] + sm.idx + p) = (j == 0 ? 1.0 : -1.0) * sm.phi[p];
                b[row] = j == 0 ? P.force_bound : 0.0;
                row++;
            }
        const double mu = P.mu_fric;
        const double pyr[4][3] = {{1, 0, -mu}, {-1, 0, -mu}, {0, 1, -mu}, {0, -1, -mu}};
        for (int s = 0; s < ns; s++) {
            const SrbmSample& sm = W.samp[s];
            for (int fc = 0; fc < 4; fc++) {
                for (int c = 0; c < 3; c++) {
                    if (pyr[fc][c] == 0) continue;
                    for (int p = 0; p < sm.cnt; p++) Aat(row, nx + W.fbase[sm.ee][c] + sm.idx + p) = pyr[fc][c] * sm.phi[p];
                }
                b[row] = 0;
                row++;
            }
        }
        // foot box (msrb.cpp:381-443; qp_data.cpp:240)
        for (int i = 0; i < 2; i++)
            for (int k = 4; k <= N; k++)
                for (int ee = 0; ee < SRBM_NEE; ee++)
                    for (int c = 0; c < 2; c++) {
                        const SrbmNodeRec& r = W.node[k][ee];
                        Aat(row, 12 * k + c) = (i == 0) ? -1 : 1;
                        for (int p = 0; p < r.pcnt; p++) Aat(row, nx + W.pbase[ee][c] + r.pidx + p) = (i == 0) ? r.plin[p] : -r.plin[p];
                        const double half = W.box_used[c] / 2, hip = P.hip[2 * ee + c];
                        b[row] = (i == 0) ? (half + hip) : -(-half + hip);
                        row++;
                    }
        // TD rows then start rows
        for (int e = 0; e < W.n_td + 8; e++) {
            for (int p = 0; p < W.eq_cnt[e]; p++) Aat(row, nx + W.eq_idx[e] + p) = W.eq_coef[e][p];
            b[row] = W.eq_rhs[e];
            row++;
        }
        if (row != m) return fail("srbm_export_qp: row count mismatch");
    }
    if (Pm && q) {
        for (int k = 0; k <= N; k++) {
            const double* Qk = (k == N) ? P.Phi : P.Q;
            const double* wk = (k == N) ? P.Phi_w : P.w;
            for (int i = 0; i < 12; i++) {
                for (int j = 0; j < 12; j++) Pm[(size_t)(12 * k + i) * n + 12 * k + j] += Qk[12 * i + j];
                q[12 * k + i] = wk[i];
            }
        }
        for (int j = 0; j < W.nf; j++) Pm[(size_t)(nx + j) * n + nx + j] += P.force_cost;
        for (int i = 0; i < n; i++) Pm[(size_t)i * n + i] += 1e-3;
    }
    return 0;
}

// ---------------- mpc::Trajectory as a flat record ----------------
static void inst_to_record(const SrbmParams& P, const SrbmInst& I, srbm_trajectory* t) {
    std::memset(t, 0, sizeof(*t));
    t->num_states = P.N + 1;
    t->init_time = I.init_time; t->node_dt = P.dt; t->swing_height = P.swing_height; t->foot_offset = P.foot_offset;
    for (int k = 0; k <= P.N; k++) std::memcpy(t->states[k], &I.states[k * 13], sizeof(double) * 13);
    for (int ee = 0; ee < SRBM_NEE; ee++) {
        t->nk[ee] = I.nk[ee];
        for (int k = 0; k < SRBM_KMAX; k++) { t->knot_kind[ee][k] = I.kind[ee][k]; t->knot_time[ee][k] = I.knot_t[ee][k]; }
    }
    static_assert(SRBM_TRAJ_KMAX == SRBM_KMAX, "record and device knot capacity agree");
    std::memcpy(t->force, I.fval, sizeof(I.fval));
    std::memcpy(t->pos_xy, I.pval, sizeof(I.pval));
}
static const char* check_record(const SrbmParams& P, const srbm_trajectory& t) {
    if (t.num_states != P.N + 1) return "num_states != num_nodes + 1";
    for (int ee = 0; ee < SRBM_NEE; ee++) {
        if (t.nk[ee] < 2 || t.nk[ee] > SRBM_KMAX) return "knot count out of range";
        int contacts = 0;
        for (int k = 0; k < t.nk[ee]; k++) {
            if (t.knot_kind[ee][k] < 0 || t.knot_kind[ee][k] > SRBM_K_MID) return "unknown knot kind";
            if (k > 0 && !(t.knot_time[ee][k] >= t.knot_time[ee][k - 1])) return "knot times must be non-decreasing";
            contacts += t.knot_kind[ee][k] <= SRBM_K_TD;
        }
        if (contacts < 2) return "a foot needs at least two contact knots";
        if (t.knot_kind[ee][0] > SRBM_K_TD) return "the first knot of a foot must be a contact knot";
    }
    return nullptr;
}
int srbm_sizeof_trajectory(void) { return (int)sizeof(srbm_trajectory); }
int srbm_get_trajectory(srbm_batch* h, int first, int count, srbm_trajectory* out) {
    if (!h || !out || first < 0 || count < 0 || first + count > h->batch) return fail("bad arguments");
    std::vector<SrbmInst> v(count);
    if (fetch(h, {{v.data(), h->insts + first, sizeof(SrbmInst) * (size_t)count}})) return -1;
    for (int i = 0; i < count; i++) inst_to_record(h->hp, v[i], out + i);
    return 0;
}
// MPC::SetWarmStartTrajectory (mpc.cpp:110-119)
int srbm_set_warm_start_trajectory(srbm_batch* h, int first, int count, const srbm_trajectory* trajs) {
    if (!h || !trajs || first < 0 || count < 0 || first + count > h->batch) return fail("bad arguments");
    for (int i = 0; i < count; i++)
        if (const char* why = check_record(h->hp, trajs[i])) return fail("srbm_set_warm_start_trajectory: record " + std::to_string(i) + ": " + why);
    std::vector<SrbmInst> v(count);
    if (fetch(h, {{v.data(), h->insts + first, sizeof(SrbmInst) * (size_t)count}})) return -1;
    for (int i = 0; i < count; i++) {
        SrbmInst& I = v[i];
        const srbm_trajectory& t = trajs[i];
        for (int k = 0; k <= h->hp.N; k++) std::memcpy(&I.states[k * 13], t.states[k], sizeof(double) * 13);
        for (int ee = 0; ee < SRBM_NEE; ee++) {
            I.nk[ee] = t.nk[ee];
            for (int k = 0; k < SRBM_KMAX; k++) {
                const bool in = k < t.nk[ee];
                I.kind[ee][k] = in ? (uint8_t)t.knot_kind[ee][k] : 0; I.knot_t[ee][k] = in ? t.knot_time[ee][k] : 0.0;
            }
        }
        std::memcpy(I.fval, t.force, sizeof(I.fval));
        std::memcpy(I.pval, t.pos_xy, sizeof(I.pval));
        I.init_time = t.init_time;              // init_time_ = trajectory.GetTime(0)
        I.low_skip = 0; I.low_streak = 0;       // a trajectory from elsewhere: what the solver remembers of this instance's earlier QPs (the back-off of
                                                // the lower-start attempts, srbm_k3_ipm.hiph) no longer applies
    }
    HIPCHK(hipMemcpy(h->insts + first, v.data(), sizeof(SrbmInst) * (size_t)count, hipMemcpyHostToDevice));
    return 0;
}
// Trajectory::GetForce / GetEndEffectorLocation / EndEffectorSplines::IsInContact on a record: host arithmetic, the same
// functions the kernels use (srbm_spline.hiph is host + device)
int srbm_trajectory_eval(const srbm_trajectory* t, int ee, double time, double* force3, double* pos3, int* in_contact) {
    if (!t || ee < 0 || ee >= SRBM_NEE) return fail("bad arguments");
    if (t->nk[ee] < 2 || t->nk[ee] > SRBM_KMAX) return fail("srbm_trajectory_eval: malformed record");
    uint8_t kind[SRBM_KMAX];
    for (int k = 0; k < SRBM_KMAX; k++) kind[k] = (uint8_t)t->knot_kind[ee][k];
    const FootView f{t->knot_time[ee], kind, t->nk[ee]};
    int err = 0;
    if (force3) srbm_force_value(f, &t->force[ee][0][0][0], time, force3, &err);
    if (pos3) {
        srbm_posxy_value(f, &t->pos_xy[ee][0][0], time, pos3, &err);
        pos3[2] = srbm_posz_value(f, time, t->swing_height, t->foot_offset, &err);
    }
    if (in_contact) {
        const int lo = srbm_lower(f, SEL_POSXY, time, &err), up = srbm_upper(f, SEL_POSXY, time, &err);
        *in_contact = (kind[lo] == SRBM_K_TD && kind[up] == SRBM_K_LO) ? 1 : 0;
    }
    return err;
}
// Trajectory::SplinesAsVec (trajectory.cpp:429-452) of a record: the spline variables in the order of the QP's decision vector -- per foot and force
// coordinate (value, slope / FORCE_MULT) of every stance-interior knot (EndEffectorSplines::GetSplineAsQPVec over the mutable force nodes), then per foot
// and xy coordinate the mutable position nodes.  The same rules kernel 1 builds its linearisation point with (srbm_k1_assemble.hiph), host arithmetic.
int srbm_trajectory_splines_as_vec(const srbm_trajectory* t, double* out, int capacity, int* n_total, int* n_force) {
    if (!t || !out || !n_total) return fail("bad arguments");
    int nf = 0, np_ = 0;
    uint8_t kind[SRBM_NEE][SRBM_KMAX], ismut[SRBM_NEE][SRBM_KMAX];
    for (int ee = 0; ee < SRBM_NEE; ee++) {
        if (t->nk[ee] < 2 || t->nk[ee] > SRBM_KMAX) return fail("srbm_trajectory_splines_as_vec: malformed record");
        for (int k = 0; k < SRBM_KMAX; k++) kind[ee][k] = (uint8_t)t->knot_kind[ee][k];
        const FootView f{t->knot_time[ee], kind[ee], t->nk[ee]};
        for (int k = 0; k < t->nk[ee]; k++) nf += kind[ee][k] == SRBM_K_F ? 6 : 0;
        np_ += 2 * srbm_pos_mutable(f, ismut[ee]);
    }
    if (nf + np_ > capacity) return fail("srbm_trajectory_splines_as_vec: output buffer too small");
    int fi = 0, pi = nf;
    for (int ee = 0; ee < SRBM_NEE; ee++) {
        for (int c = 0; c < 3; c++) {
            for (int k = 0; k < t->nk[ee]; k++)
                if (kind[ee][k] == SRBM_K_F) { out[fi++] = t->force[ee][c][k][0]; out[fi++] = t->force[ee][c][k][1]; }
            if (c < 2)
                for (int k = 0; k < t->nk[ee]; k++) if (ismut[ee][k]) out[pi++] = t->pos_xy[ee][c][k];
        }
    }
    *n_total = nf + np_;
    if (n_force) *n_force = nf;
    return 0;
}
// SingleRigidBodyModel::ConvertManifoldStateToTangentState / ConvertTangentStateToManifoldState (single_rigid_body_model.cpp:188-220; the
// reference state argument is unused there: quat_ref is the identity): host arithmetic, the functions the kernels use
int srbm_convert_manifold_to_tangent(const double* state13, double* tangent12) {
    if (!state13 || !tangent12) return fail("bad arguments");
    srbm_manifold_to_tangent(state13, tangent12);
    return 0;
}
int srbm_convert_tangent_to_manifold(const double* tangent12, double* state13) {
    if (!tangent12 || !state13) return fail("bad arguments");
    srbm_tangent_to_manifold(tangent12, state13);
    return 0;
}
int srbm_eval_trajectory(srbm_batch* h, const double* time, double* force, double* pos, int* in_contact) {
    if (!h || !time) return fail("bad arguments");
    if (use_batch(h)) return -1;
    const size_t B = h->batch;
    Carve c;                                          // in: time; out: force, pos, in_contact
    const auto t = c.add<double>(B), f = c.add<double>(12 * B), ps = c.add<double>(12 * B);
    const auto ic = c.add<int>(4 * B);
    if (c.stage(h)) return -1;
    memcpy(c.host(t), time, t.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(t), c.host(t), t.bytes(), hipMemcpyHostToDevice, h->stream));
    if (srbm_eval_trajectory_dev(h, c.dev(t), c.dev(f), c.dev(ps), c.dev(ic))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(f), c.dev(f), Carve::span(f, ic), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (force) memcpy(force, c.host(f), f.bytes());
    if (pos) memcpy(pos, c.host(ps), ps.bytes());
    if (in_contact) memcpy(in_contact, c.host(ic), ic.bytes());
    return 0;
}
int srbm_eval_trajectory_dev(srbm_batch* h, const double* time_dev, double* force_dev, double* pos_dev, int* in_contact_dev) {
    if (!h || !time_dev || !force_dev || !pos_dev || !in_contact_dev) return fail("bad arguments");
    if (use_batch(h)) return -1;
    const int tot = h->batch * SRBM_NEE;
    hipLaunchKernelGGL(srbm_k_eval_trajectory, dim3((tot + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, time_dev, force_dev, pos_dev, in_contact_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_get_ee_box_center(const srbm_batch* h, double* centers) {
    if (!h || !centers) return fail("bad arguments");
    std::memcpy(centers, h->hp.hip, sizeof(double) * 8);
    return 0;
}
int srbm_get_cost(srbm_batch* h, double* cost) {
    if (!h || !cost) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { cost[b] = I.cost; });
}
// merit[b] = cost + mu |dynamics defect|_1 of the trajectory after the last solve (MPC::GetMeritValue, mpc.cpp:749-753, mu = 5000) and
// the directional derivative of the merit along the last step (GetMeritGradient, :783-788): the 'Merit' / 'Merit dd' columns
int srbm_get_merit(srbm_batch* h, double* merit, double* merit_dd) {
    if (!h || !merit) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { merit[b] = I.cost + h->hp.merit_mu * I.eq_violation; if (merit_dd) merit_dd[b] = I.merit_dd; });
}
int srbm_get_avg_cost(srbm_batch* h, double* avg) {
    if (!h || !avg) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { avg[b] = I.cost_sum / I.run_num; });      // (0/0 = NaN before the first solve, as the reference's)
}
int srbm_get_status_accumulated(srbm_batch* h, int* acc) {
    if (!h || !acc) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) {
        acc[4 * b] = I.err_acc | I.err; acc[4 * b + 1] = I.n_solves; acc[4 * b + 2] = I.n_not_solved; acc[4 * b + 3] = I.n_maxiter;
    });
}
int srbm_clear_status_accumulators(srbm_batch* h) {
    if (!h) return fail("bad arguments");
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_clear_acc, dim3((h->batch + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_get_solver_counters(srbm_batch* h, long long* c4) {
    if (!h || !c4) return fail("bad arguments");
    long long c[4] = {0, 0, 0, 0};
    if (each_inst(h, [&](int, const SrbmInst& I) { c[0] += I.n_solves; c[1] += I.n_step_rule; c[2] += I.n_low_tried; c[3] += I.n_low_failed; })) return -1;
    std::memcpy(c4, c, sizeof(c));
    return 0;
}
int srbm_get_solve_flags(srbm_batch* h, int* flags) {
    if (!h || !flags) return fail("bad arguments");
    return each_inst(h, [&](int b, const SrbmInst& I) { flags[b] = (I.last_rule ? 1 : 0) | ((I.last_low & 1) ? 2 : 0) | ((I.last_low & 2) ? 4 : 0); });
}
int srbm_result_record_doubles(int N) { return 8 + 12 * (N + 1) + SRBM_NUMAX + 12 * (N + 1) + 6 * SRBM_NSMAX + 16 * (N - 3) + 16 + 36; }
int srbm_get_executed_mfma(srbm_batch* h, double* total) {
    if (!h || !total) return fail("bad arguments");
    double t = 0;
    if (each_inst(h, [&](int, const SrbmInst& I) { t += I.acc_mfma; })) return -1;
    *total = t;
    return 0;
}

// ---------------- row f3: whole-body targets ----------------
int srbm_set_leg_kinematics(srbm_batch* h, const srbm_leg_kinematics* legs) {
    if (!h || !legs) return fail("bad arguments");
    std::memcpy(h->hp.legs, legs->origin, sizeof(h->hp.legs));
    h->hp.has_legs = 1;
    params_changed(h);
    return 0;
}
static int need_legs(srbm_batch* h) { return h->hp.has_legs ? 0 : fail("the leg geometry has not been set (srbm_set_leg_kinematics)"); }
int srbm_forward_kinematics(srbm_batch* h, const double* q, double* ee) {
    if (!h || !q || !ee) return fail("bad arguments");
    if (need_legs(h) || use_batch(h)) return -1;
    const size_t B = h->batch;
    Carve c;
    const auto dq = c.add<double>(19 * B), de = c.add<double>(12 * B);
    if (c.scratch(h)) return -1;
    HIPCHK(hipMemcpyAsync(c.dev(dq), q, dq.bytes(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(srbm_k_forward_kinematics, dim3((h->batch + 63) / 64), dim3(64), 0, h->stream, h->dp, c.dev(dq), c.dev(de));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(ee, c.dev(de), de.bytes(), hipMemcpyDeviceToHost));
    return 0;
}
int srbm_inverse_kinematics(srbm_batch* h, const double* state, const double* ee, const double* q_guess, double* q_out, int* iters, int* status) {
    if (!h || !state || !ee || !q_guess || !q_out) return fail("bad arguments");
    if (need_legs(h) || use_batch(h)) return -1;
    const size_t B = h->batch;
    Carve c;
    const auto ds = c.add<double>(13 * B), de = c.add<double>(12 * B), dg = c.add<double>(19 * B), dq = c.add<double>(19 * B);
    const auto di = c.add<int>(4 * B), dst = c.add<int>(B);
    if (c.scratch(h)) return -1;
    HIPCHK(hipMemcpyAsync(c.dev(ds), state, ds.bytes(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(c.dev(de), ee, de.bytes(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(c.dev(dg), q_guess, dg.bytes(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(srbm_k_inverse_kinematics, dim3(h->batch), dim3(SRBM_IK_THREADS), 0, h->stream, h->dp, c.dev(ds), c.dev(de), c.dev(dg), c.dev(dq),
                       c.dev(di), c.dev(dst));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return copy_each({{q_out, c.dev(dq), dq.bytes()}, {iters, c.dev(di), di.bytes()}, {status, c.dev(dst), dst.bytes()}}, hipMemcpyDeviceToHost);
}
int srbm_get_targets_from_traj(srbm_batch* h, const double* time, double* q_des, double* v_des, double* force_des, int* status) {
    if (!h || !time || !q_des || !v_des || !force_des) return fail("bad arguments");
    if (need_legs(h) || use_batch(h)) return -1;
    const size_t B = h->batch;
    Carve c;                                          // in: time, q_des (the guess); out: q_des, v_des, force_des, status
    const auto t = c.add<double>(B), q = c.add<double>(19 * B), v = c.add<double>(18 * B), f = c.add<double>(12 * B);
    const auto st = c.add<int>(B);
    if (c.stage(h)) return -1;
    memcpy(c.host(t), time, t.bytes());
    memcpy(c.host(q), q_des, q.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(t), c.host(t), Carve::span(t, q), hipMemcpyHostToDevice, h->stream));
    if (srbm_get_targets_from_traj_dev(h, c.dev(t), c.dev(q), c.dev(v), c.dev(f), c.dev(st))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(q), c.dev(q), Carve::span(q, st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(q_des, c.host(q), q.bytes());
    memcpy(v_des, c.host(v), v.bytes());
    memcpy(force_des, c.host(f), f.bytes());
    if (status) memcpy(status, c.host(st), st.bytes());
    return 0;
}

// the same on device pointers: one launch on the batch's stream, no copy, no synchronisation (a control tick of the whole batch stays in HBM)
int srbm_get_targets_from_traj_dev(srbm_batch* h, const double* time_dev, double* q_des_dev, double* v_des_dev, double* force_des_dev, int* status_dev) {
    if (!h || !time_dev || !q_des_dev || !v_des_dev || !force_des_dev || !status_dev) return fail("bad arguments");
    if (need_legs(h) || use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_targets_from_traj, dim3(h->batch), dim3(SRBM_TT_THREADS), 0, h->stream, h->dp, h->insts, time_dev, q_des_dev, v_des_dev, force_des_dev, status_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

int srbm_set_wbc_model(srbm_batch* h, const srbm_wbc_model* m) {
    if (!h || !m) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    SrbmWbcParams w;
    for (int b = 0; b < 13; b++) {
        w.body[b].mass = m->body_mass[b];
        for (int i = 0; i < 3; i++) w.body[b].com[i] = m->body_com[b][i];
        for (int i = 0; i < 9; i++) w.body[b].I[i] = m->body_inertia[b][i];
    }
    for (int i = 0; i < 12; i++) { w.torque_bounds[i] = m->torque_bounds[i]; w.kp_joint[i] = m->kp_joint_gains[i]; w.kd_joint[i] = m->kd_joint_gains[i]; }
    w.kv_pos = m->base_pos_gains[0]; w.kp_pos = m->base_pos_gains[1]; w.kv_ang = m->base_ang_gains[0]; w.kp_ang = m->base_ang_gains[1];
    w.leg_weight = m->leg_tracking_weight; w.torso_weight = m->torso_tracking_weight; w.force_weight = m->force_tracking_weight;
    w.friction = m->friction_coef; w.max_grf = m->max_grf;
    if (!h->d_wbc) HIPCHK(hipMalloc(&h->d_wbc, sizeof(SrbmWbcParams)));
    HIPCHK(hipMemcpy(h->d_wbc, &w, sizeof(w), hipMemcpyHostToDevice));
    return 0;
}
int srbm_qp_control(srbm_batch* h, const double* q, const double* v, const int* contact, const double* q_des, const double* v_des,
                    const double* force_des, double* control, double* qp_sol, int* status, double* qp_dump) {
    if (!h || !q || !v || !contact || !q_des || !v_des || !force_des || !control) return fail("bad arguments");
    if (need_legs(h)) return -1;
    if (!h->d_wbc) return fail("the whole-body model has not been set (srbm_set_wbc_model)");
    if (use_batch(h)) return -1;
    const size_t B = h->batch, DUMP = WBC_MMAX * WBC_NMAX + 2 * WBC_MMAX + 2 * WBC_NMAX;
    Carve c;                                          // in: q, v, q_des, v_des, force_des, contact; out: control, qp_sol, status, the optional dump
    const auto iq = c.add<double>(19 * B), iv = c.add<double>(18 * B), iqd = c.add<double>(19 * B), ivd = c.add<double>(18 * B), ifd = c.add<double>(12 * B);
    const auto icon = c.add<int>(4 * B);
    const auto oc = c.add<double>(36 * B), os = c.add<double>(WBC_NMAX * B);
    const auto ost = c.add<int>(B);
    const auto od = c.add<double>(qp_dump ? DUMP * B : 0);
    if (c.stage(h)) return -1;
    memcpy(c.host(iq), q, iq.bytes());
    memcpy(c.host(iv), v, iv.bytes());
    memcpy(c.host(iqd), q_des, iqd.bytes());
    memcpy(c.host(ivd), v_des, ivd.bytes());
    memcpy(c.host(ifd), force_des, ifd.bytes());
    memcpy(c.host(icon), contact, icon.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(iq), c.host(iq), Carve::span(iq, icon), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(srbm_k_qp_control, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, h->d_wbc, c.dev(iq), c.dev(iv), c.dev(icon), c.dev(iqd),
                       c.dev(ivd), c.dev(ifd), c.dev(oc), c.dev(os), c.dev(ost), qp_dump ? c.dev(od) : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.host(oc), c.dev(oc), Carve::span(oc, od), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(control, c.host(oc), oc.bytes());
    if (qp_sol) memcpy(qp_sol, c.host(os), os.bytes());
    if (status) memcpy(status, c.host(ost), ost.bytes());
    if (qp_dump) memcpy(qp_dump, c.host(od), od.bytes());
    return 0;
}

int srbm_qp_control_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const int* contact_dev, const double* q_des_dev, const double* v_des_dev,
                        const double* force_des_dev, double* control_dev, double* qp_sol_dev, int* status_dev) {
    if (!h || !q_dev || !v_dev || !contact_dev || !q_des_dev || !v_des_dev || !force_des_dev || !control_dev || !qp_sol_dev || !status_dev) return fail("bad arguments");
    if (need_legs(h)) return -1;
    if (!h->d_wbc) return fail("the whole-body model has not been set (srbm_set_wbc_model)");
    if (use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_qp_control, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, h->d_wbc, q_dev, v_dev, contact_dev, q_des_dev, v_des_dev,
                       force_des_dev, control_dev, qp_sol_dev, status_dev, static_cast<double*>(nullptr));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------- the control tick as one entry (srbm_tick.hiph) ----------------
// what both entries need, asked before anything is staged, copied or launched
static int tick_usable(srbm_batch* h) {
    if (need_legs(h)) return -1;
    if (!h->d_wbc) return fail("the whole-body model has not been set (srbm_set_wbc_model)");
    if (!h->d_tick_q) return fail("srbm_control_tick: q_des has not been set (srbm_control_tick_reset: the IK guess of the first tick)");
    return 0;
}
int srbm_control_tick_reset(srbm_batch* h, const double* q_des) {
    if (!h || !q_des) return fail("srbm_control_tick_reset: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (tick_alloc(h)) return -1;
    HIPCHK(hipMemcpyAsync(h->d_tick_q, q_des, sizeof(double) * 19 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_control_tick_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* time_dev, double* control_dev, double* qp_sol_dev, int* status_dev,
                          double* q_des_dev, double* v_des_dev, int* contact_dev, double* state_dev, double* ee_dev) {
    if (!h || !q_dev || !v_dev || !time_dev || !control_dev || !qp_sol_dev || !status_dev) return fail("srbm_control_tick: bad arguments");
    if (tick_usable(h) || use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_tick_targets, dim3(h->batch), dim3(SRBM_TT_THREADS), 0, h->stream, h->dp, h->pub_insts ? h->pub_insts : h->insts, time_dev, h->d_tick_q,
                       h->d_tick_rec);          // (with a latency set: the published trajectories)
    const SrbmTickIO io{q_dev, v_dev, time_dev, control_dev, qp_sol_dev, status_dev, q_des_dev, v_des_dev, contact_dev, state_dev, ee_dev};
    hipLaunchKernelGGL(srbm_k_tick_control, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, h->d_wbc, h->d_tick_rec, h->d_tick_q, io);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_control_tick(srbm_batch* h, const double* q, const double* v, const double* time, double* control, double* qp_sol, int* status, double* q_des,
                      double* v_des, int* contact, double* state, double* ee) {
    if (!h || !q || !v || !time || !control || !qp_sol || !status) return fail("srbm_control_tick: bad arguments");
    if (tick_usable(h)) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    Carve c;                                          // in: q, v, time; out: control .. ee
    const auto iq = c.add<double>(19 * B), iv = c.add<double>(18 * B), it = c.add<double>(B);
    const auto oc = c.add<double>(36 * B), os = c.add<double>(WBC_NMAX * B), oq = c.add<double>(19 * B), ov = c.add<double>(18 * B), ox = c.add<double>(13 * B),
               oe = c.add<double>(12 * B);
    const auto ost = c.add<int>(2 * B), ocon = c.add<int>(4 * B);
    if (c.stage(h)) return -1;
    memcpy(c.host(iq), q, iq.bytes());
    memcpy(c.host(iv), v, iv.bytes());
    memcpy(c.host(it), time, it.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(iq), c.host(iq), Carve::span(iq, it), hipMemcpyHostToDevice, h->stream));
    if (srbm_control_tick_dev(h, c.dev(iq), c.dev(iv), c.dev(it), c.dev(oc), c.dev(os), c.dev(ost), c.dev(oq), c.dev(ov), c.dev(ocon), c.dev(ox), c.dev(oe))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(oc), c.dev(oc), Carve::span(oc, ocon), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(control, c.host(oc), oc.bytes());
    memcpy(qp_sol, c.host(os), os.bytes());
    memcpy(status, c.host(ost), ost.bytes());
    if (q_des) memcpy(q_des, c.host(oq), oq.bytes());
    if (v_des) memcpy(v_des, c.host(ov), ov.bytes());
    if (contact) memcpy(contact, c.host(ocon), ocon.bytes());
    if (state) memcpy(state, c.host(ox), ox.bytes());
    if (ee) memcpy(ee, c.host(oe), oe.bytes());
    return 0;
}

// ---------------- whole-controller rollouts: MPC updates, control ticks, whole-body plant (srbm_wb_plant.hiph) ----------------
// with a latency set: the published trajectories and the latency record as srbm_controller_set_latency leaves them, on the stream
static int latency_resync(srbm_batch* h) {
    if (!h->pub_insts) return 0;
    HIPCHK(hipMemcpyAsync(h->pub_insts, h->insts, sizeof(SrbmInst) * (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_pub, h->pub_init.data(), sizeof(double) * h->pub_init.size(), hipMemcpyHostToDevice, h->stream));
    return 0;
}
// with sensors set: the sensor state of a plant at (q, v) (host arrays), the record of the run zeroed, the last measurement (q, v); synchronous
static int sensors_reinit(srbm_batch* h, const double* q, const double* v) {
    if (!h->d_sens) return 0;
    const size_t B = h->batch;
    const SensBuf s = sens_buf(h);
    std::vector<double> ms(SRBM_SENS_STATE_DOUBLES * B);
    for (size_t b = 0; b < B; b++) srbm_sensor_state_init(q + 19 * b, v + 18 * b, ms.data() + SRBM_SENS_STATE_DOUBLES * b);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(s.ms, ms.data(), sizeof(double) * ms.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s.srec, 0, sizeof(double) * SRBM_SENS_RECORD_DOUBLES * B));
    HIPCHK(hipMemcpy(s.qm, q, sizeof(double) * 19 * B, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.vm, v, sizeof(double) * 18 * B, hipMemcpyHostToDevice));
    h->sens_ready = true;
    return 0;
}
int srbm_wb_plant_set_state(srbm_batch* h, const double* q, const double* v) {
    if (!h || !q || !v) return fail("srbm_wb_plant_set_state: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (wb_alloc(h)) return -1;
    const WbBuf w = wb_buf(h);
    HIPCHK(hipMemcpyAsync(w.q, q, sizeof(double) * 19 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(w.v, v, sizeof(double) * 18 * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_cs, 0, sizeof(double) * WBG_CS_DOUBLES * (size_t)h->batch, h->stream));          // no foot in contact
    if (h->d_joints) HIPCHK(hipMemsetAsync(joint_buf(h).js, 0, sizeof(double) * (12 + WBJ_RECORD_DOUBLES) * (size_t)h->batch, h->stream));   // motors at rest, record empty
    if (h->d_wrench) HIPCHK(hipMemsetAsync(wrench_buf(h).wrec, 0, sizeof(double) * WBW_RECORD_DOUBLES * (size_t)h->batch, h->stream));
    if (h->d_cmd) HIPCHK(hipMemcpyAsync(cmd_buf(h).cstate, h->cmd_init.data(), sizeof(double) * h->cmd_init.size(), hipMemcpyHostToDevice, h->stream));   // nothing latched
    std::vector<double> fb(SRBM_FB_DOUBLES * (size_t)h->batch);                                                   // no touch-down moved
    for (size_t i = 0; i < fb.size(); i++) fb[i] = i % 2 ? -1.0 : 0.0;
    HIPCHK(hipMemcpyAsync(h->d_fb, fb.data(), sizeof(double) * fb.size(), hipMemcpyHostToDevice, h->stream));
    if (latency_resync(h)) return -1;                                                                             // what is in force: what the MPC holds now
    if (srbm_synchronize(h)) return -1;          // (fb is read until here)
    return sensors_reinit(h, q, v);
}
int srbm_wb_plant_get_state(srbm_batch* h, double* q, double* v) {
    if (!h) return fail("srbm_wb_plant_get_state: bad arguments");
    if (!h->d_wb) return fail("the whole-body plant state has not been set (srbm_wb_plant_set_state)");
    const WbBuf w = wb_buf(h);
    return fetch(h, {{q, w.q, sizeof(double) * 19 * (size_t)h->batch}, {v, w.v, sizeof(double) * 18 * (size_t)h->batch}});
}
// the refusal of a tick the step entries cannot run
static int check_tick(const char* fn, int tick, double tick_dt) {
    if (tick < 0 || !std::isfinite(tick_dt) || tick_dt <= 0.0) return fail(std::string(fn) + ": tick >= 0 and a finite tick_dt > 0 are required");
    return 0;
}
// the plant step of tick `tick` on the batch's stream; lg: the record of the tick, nullptr: the unlogged kernel
static int launch_wb_plant(srbm_batch* h, int tick, double tick_dt, double* q, double* v, const double* qp_sol, const int* status, double* time_next,
                           const SrbmTickLogArgs* lg) {
    const double* push = h->push_set ? h->d_push : nullptr;
    if (lg) hipLaunchKernelGGL((srbm_k_wb_plant_step<true>), dim3(h->batch), dim3(64), 0, h->stream, h->dp, tick, tick_dt, push, q, v, qp_sol, status, time_next, *lg);
    else hipLaunchKernelGGL((srbm_k_wb_plant_step<false>), dim3(h->batch), dim3(64), 0, h->stream, h->dp, tick, tick_dt, push, q, v, qp_sol, status, time_next,
                            SrbmTickLogArgs{nullptr, nullptr, nullptr, nullptr, 0});
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_wb_plant_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, const double* qp_sol_dev, const int* status_dev) {
    if (!h || !q_dev || !v_dev || !qp_sol_dev || !status_dev) return fail("srbm_wb_plant_step_dev: bad arguments");
    if (check_tick("srbm_wb_plant_step_dev", tick, tick_dt) || use_batch(h)) return -1;
    return launch_wb_plant(h, tick, tick_dt, q_dev, v_dev, qp_sol_dev, status_dev, nullptr, nullptr);
}
// ---- the torque-driven plant (srbm_wb_fd.hiph) ----
static const char* const FD_NO_ACTUATORS = "the torque-driven plant has no actuators (srbm_wb_plant_set_actuators)";
int srbm_wb_plant_set_kind(srbm_batch* h, int kind) {
    if (!h) return fail("srbm_wb_plant_set_kind: bad arguments");
    if (kind != 0 && kind != 1) return fail("srbm_wb_plant_set_kind: kind " + std::to_string(kind) + " (0: the QP-acceleration plant, 1: the torque-driven plant)");
    h->fd_kind = kind;
    return 0;
}
int srbm_wb_plant_set_actuators(srbm_batch* h, const double* kp, const double* kd, const double* torque_limit, int substeps) {
    const std::string fn = "srbm_wb_plant_set_actuators";
    if (!h || !kp || !kd || !torque_limit) return fail(fn + ": bad arguments");
    if (substeps < 1) return fail(fn + ": substeps >= 1 is required");
    const size_t B = h->batch;
    for (size_t e = 0; e < 12 * B; e++) {
        const std::string at = fn + ": instance " + std::to_string(e / 12) + ", joint " + std::to_string(e % 12) + ": ";
        if (!std::isfinite(kp[e]) || kp[e] < 0.0) return fail(at + "kp must be finite and >= 0");
        if (!std::isfinite(kd[e]) || kd[e] < 0.0) return fail(at + "kd must be finite and >= 0");
        if (!(torque_limit[e] >= 0.0)) return fail(at + "the torque limit must be >= 0 (+inf: none)");
    }
    HIPCHK(hipSetDevice(h->device));
    Carve c;
    const auto a = c.add<double>(WBFD_ACT_DOUBLES * B);
    if (c.stage(h)) return -1;
    if (!h->d_fd_act) HIPCHK(hipMalloc(&h->d_fd_act, a.bytes()));
    double* dst = c.host(a);
    for (size_t b = 0; b < B; b++) {
        std::memcpy(dst + WBFD_ACT_DOUBLES * b, kp + 12 * b, sizeof(double) * 12);
        std::memcpy(dst + WBFD_ACT_DOUBLES * b + 12, kd + 12 * b, sizeof(double) * 12);
        std::memcpy(dst + WBFD_ACT_DOUBLES * b + 24, torque_limit + 12 * b, sizeof(double) * 12);
    }
    HIPCHK(hipMemcpyAsync(h->d_fd_act, dst, a.bytes(), hipMemcpyHostToDevice, h->stream));
    h->fd_substeps = substeps;
    return srbm_synchronize(h);
}
int srbm_wb_plant_set_bodies_each(srbm_batch* h, const double* body_mass, const double* body_com, const double* body_inertia) {
    const std::string fn = "srbm_wb_plant_set_bodies_each";
    if (!h || !body_mass || !body_com || !body_inertia) return fail(fn + ": bad arguments");
    const size_t B = h->batch;
    for (size_t e = 0; e < 13 * B; e++) {
        const std::string at = fn + ": instance " + std::to_string(e / 13) + ", body " + std::to_string(e % 13) + ": ";
        if (!std::isfinite(body_mass[e]) || body_mass[e] <= 0.0) return fail(at + "the mass must be finite and > 0");
        for (int i = 0; i < 3; i++) if (!std::isfinite(body_com[3 * e + i])) return fail(at + "the centre of mass is not finite");
        for (int i = 0; i < 9; i++) if (!std::isfinite(body_inertia[9 * e + i])) return fail(at + "the inertia is not finite");
    }
    HIPCHK(hipSetDevice(h->device));
    Carve c;
    const auto a = c.add<SrbmBody>(13 * B);
    if (c.stage(h)) return -1;
    if (!h->d_fd_bodies) HIPCHK(hipMalloc(&h->d_fd_bodies, a.bytes()));
    SrbmBody* dst = c.host(a);
    for (size_t e = 0; e < 13 * B; e++) {
        dst[e].mass = body_mass[e];
        std::memcpy(dst[e].com, body_com + 3 * e, sizeof(double) * 3);
        std::memcpy(dst[e].I, body_inertia + 9 * e, sizeof(double) * 9);
    }
    HIPCHK(hipMemcpyAsync(h->d_fd_bodies, dst, a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
// the plant's bodies and their stride per instance: its own, or the controller's for every instance
static const SrbmBody* fd_bodies(const srbm_batch* h, int* stride) {
    *stride = h->d_fd_bodies ? 13 : 0;
    return h->d_fd_bodies ? h->d_fd_bodies : reinterpret_cast<const SrbmBody*>(h->d_wbc);
}
static int fd_usable(srbm_batch* h, const char* fn) {
    if (need_legs(h)) return -1;
    if (!h->d_wbc && !h->d_fd_bodies)
        return fail(std::string(fn) + ": the whole-body model has not been set (srbm_set_wbc_model), and the plant has no bodies of its own (srbm_wb_plant_set_bodies_each)");
    return 0;
}
// the torque-driven plant step of tick `tick` on the batch's stream: on the ground with the contact state cs, with the feet of `contact` held where
// cs is nullptr; contact (on a ground: the plan's) and qp_sol are the tick's, for the record; lg: the record of the tick, nullptr: the unlogged kernel.
// On a ground with a terrain in force (terrain_in_force) the step is the terrain's
static bool terrain_in_force(const srbm_batch* h) { return h->fd_kind == 1 && h->d_ground && h->d_terrain; }
// With a joint model in force (joints_in_force) every step and every solve of kind 1 is the joint model's instantiation (srbm_wb_joints.hiph)
static bool joints_in_force(const srbm_batch* h) { return h->fd_kind == 1 && h->d_joints; }
// With a wrench schedule in force (wrenches_in_force) every step of kind 1 is the schedule's instantiation (srbm_wb_wrench.hiph), with or without the
// joint model's law
static bool wrenches_in_force(const srbm_batch* h) { return h->fd_kind == 1 && h->d_wrench; }
static int launch_wb_torque(srbm_batch* h, int tick, double tick_dt, double* q, double* v, double* cs, const double* control, const int* contact, const int* status,
                            const double* qp_sol, double* sol_out, double* time_next, const SrbmTickLogArgs* lg) {
    const double* push = h->push_set ? h->d_push : nullptr;
    int stride = 0;
    const SrbmBody* bodies = fd_bodies(h, &stride);
    const SrbmFdArgs fa{bodies, stride, h->d_fd_act, h->fd_substeps, control, contact, qp_sol, sol_out};
    const SrbmGroundArgs ga{h->d_ground, cs};
    const SrbmTickLogArgs l = lg ? *lg : SrbmTickLogArgs{nullptr, nullptr, nullptr, nullptr, 0};
    const dim3 grid(h->batch), block(WBC_THREADS);
    if (wrenches_in_force(h)) {
        const bool jn = joints_in_force(h);
        const JointBuf jb = jn ? joint_buf(h) : JointBuf{nullptr, nullptr, nullptr, nullptr};
        const SrbmJointArgs ja{jb.joints, jb.stops, jb.js, jb.jrec};
        const SrbmWrenchArgs wa = wrench_buf(h);
        // (LOGGED, JOINTS) -> the instantiation
        #define WRENCH_STEP(K, ...) do { \
            if (lg && jn) hipLaunchKernelGGL((K<true, true>), grid, block, 0, h->stream, __VA_ARGS__); \
            else if (lg) hipLaunchKernelGGL((K<true, false>), grid, block, 0, h->stream, __VA_ARGS__); \
            else if (jn) hipLaunchKernelGGL((K<false, true>), grid, block, 0, h->stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((K<false, false>), grid, block, 0, h->stream, __VA_ARGS__); } while (0)
        if (cs && terrain_in_force(h)) WRENCH_STEP(srbm_k_wb_terrain_wrench_step, h->dp, fa, ga, h->d_terrain, ja, wa, tick, tick_dt, push, q, v, status, time_next, l);
        else if (cs) WRENCH_STEP(srbm_k_wb_ground_wrench_step, h->dp, fa, ga, ja, wa, tick, tick_dt, push, q, v, status, time_next, l);
        else WRENCH_STEP(srbm_k_wb_fd_wrench_step, h->dp, fa, ja, wa, tick, tick_dt, push, q, v, status, time_next, l);
        #undef WRENCH_STEP
    }
    else if (joints_in_force(h)) {
        const JointBuf jb = joint_buf(h);
        const SrbmJointArgs ja{jb.joints, jb.stops, jb.js, jb.jrec};
        if (cs && terrain_in_force(h)) {
            if (lg) hipLaunchKernelGGL((srbm_k_wb_terrain_joint_step<true>), grid, block, 0, h->stream, h->dp, fa, ga, h->d_terrain, ja, tick, tick_dt, push, q, v, status, time_next, l);
            else hipLaunchKernelGGL((srbm_k_wb_terrain_joint_step<false>), grid, block, 0, h->stream, h->dp, fa, ga, h->d_terrain, ja, tick, tick_dt, push, q, v, status, time_next, l);
        }
        else if (cs && lg) hipLaunchKernelGGL((srbm_k_wb_ground_joint_step<true>), grid, block, 0, h->stream, h->dp, fa, ga, ja, tick, tick_dt, push, q, v, status, time_next, l);
        else if (cs) hipLaunchKernelGGL((srbm_k_wb_ground_joint_step<false>), grid, block, 0, h->stream, h->dp, fa, ga, ja, tick, tick_dt, push, q, v, status, time_next, l);
        else if (lg) hipLaunchKernelGGL((srbm_k_wb_fd_joint_step<true>), grid, block, 0, h->stream, h->dp, fa, ja, tick, tick_dt, push, q, v, status, time_next, l);
        else hipLaunchKernelGGL((srbm_k_wb_fd_joint_step<false>), grid, block, 0, h->stream, h->dp, fa, ja, tick, tick_dt, push, q, v, status, time_next, l);
    }
    else if (cs && terrain_in_force(h)) {
        if (lg) hipLaunchKernelGGL((srbm_k_wb_terrain_step<true>), grid, block, 0, h->stream, h->dp, fa, ga, h->d_terrain, tick, tick_dt, push, q, v, status, time_next, l);
        else hipLaunchKernelGGL((srbm_k_wb_terrain_step<false>), grid, block, 0, h->stream, h->dp, fa, ga, h->d_terrain, tick, tick_dt, push, q, v, status, time_next, l);
    }
    else if (cs && lg) hipLaunchKernelGGL((srbm_k_wb_ground_step<true>), grid, block, 0, h->stream, h->dp, fa, ga, tick, tick_dt, push, q, v, status, time_next, l);
    else if (cs) hipLaunchKernelGGL((srbm_k_wb_ground_step<false>), grid, block, 0, h->stream, h->dp, fa, ga, tick, tick_dt, push, q, v, status, time_next, l);
    else if (lg) hipLaunchKernelGGL((srbm_k_wb_fd_step<true>), grid, block, 0, h->stream, h->dp, fa, tick, tick_dt, push, q, v, status, time_next, l);
    else hipLaunchKernelGGL((srbm_k_wb_fd_step<false>), grid, block, 0, h->stream, h->dp, fa, tick, tick_dt, push, q, v, status, time_next, l);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_wb_forward_dynamics_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* tau_dev, const int* contact_dev, double* sol_dev, int* status_dev) {
    if (!h || !q_dev || !v_dev || !tau_dev || !contact_dev || !sol_dev || !status_dev) return fail("srbm_wb_forward_dynamics: bad arguments");
    if (fd_usable(h, "srbm_wb_forward_dynamics") || use_batch(h)) return -1;
    int stride = 0;
    const SrbmBody* bodies = fd_bodies(h, &stride);
    if (joints_in_force(h))
        hipLaunchKernelGGL(srbm_k_wb_forward_dynamics_joint, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, h->d_joints, q_dev, v_dev, tau_dev,
                           contact_dev, sol_dev, status_dev);
    else
        hipLaunchKernelGGL(srbm_k_wb_forward_dynamics, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, q_dev, v_dev, tau_dev, contact_dev, sol_dev, status_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_wb_forward_dynamics(srbm_batch* h, const double* q, const double* v, const double* tau, const int* contact, double* sol, int* status) {
    if (!h || !q || !v || !tau || !contact || !sol) return fail("srbm_wb_forward_dynamics: bad arguments");
    if (fd_usable(h, "srbm_wb_forward_dynamics")) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    Carve c;                                          // in: q, v, tau, contact; out: sol, status
    const auto iq = c.add<double>(19 * B), iv = c.add<double>(18 * B), it = c.add<double>(12 * B);
    const auto icon = c.add<int>(4 * B);
    const auto os = c.add<double>(WBC_NMAX * B);
    const auto ost = c.add<int>(B);
    if (c.stage(h)) return -1;
    memcpy(c.host(iq), q, iq.bytes());
    memcpy(c.host(iv), v, iv.bytes());
    memcpy(c.host(it), tau, it.bytes());
    memcpy(c.host(icon), contact, icon.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(iq), c.host(iq), Carve::span(iq, icon), hipMemcpyHostToDevice, h->stream));
    if (srbm_wb_forward_dynamics_dev(h, c.dev(iq), c.dev(iv), c.dev(it), c.dev(icon), c.dev(os), c.dev(ost))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(os), c.dev(os), Carve::span(os, ost), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(sol, c.host(os), os.bytes());
    if (status) memcpy(status, c.host(ost), ost.bytes());
    return 0;
}
int srbm_wb_fd_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, const double* control_dev, const int* contact_dev,
                        const int* status_dev, double* sol_dev) {
    if (!h || !q_dev || !v_dev || !control_dev || !contact_dev || !status_dev) return fail("srbm_wb_fd_step_dev: bad arguments");
    if (check_tick("srbm_wb_fd_step_dev", tick, tick_dt) || fd_usable(h, "srbm_wb_fd_step_dev")) return -1;
    if (!h->d_fd_act) return fail(std::string("srbm_wb_fd_step_dev: ") + FD_NO_ACTUATORS);
    if (use_batch(h)) return -1;
    return launch_wb_torque(h, tick, tick_dt, q_dev, v_dev, nullptr, control_dev, contact_dev, status_dev, nullptr, sol_dev, nullptr, nullptr);
}
// ---- the ground of the torque-driven plant (srbm_wb_ground.hiph) ----
static const char* const WB_NO_STATE = "the whole-body plant state has not been set (srbm_wb_plant_set_state)";
int srbm_wb_plant_set_ground(srbm_batch* h, const double* ground) {
    const std::string fn = "srbm_wb_plant_set_ground";
    if (!h) return fail(fn + ": bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (!ground) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_ground) HIPCHK(hipFree(h->d_ground));
        h->d_ground = nullptr;
        return 0;
    }
    const size_t B = h->batch;
    static const char* const names[WBG_GROUND_DOUBLES] = {"the ground height", "the normal stiffness", "the normal damping", "the friction coefficient",
                                                          "the tangential stiffness", "the tangential damping", "reserved", "reserved"};
    for (size_t e = 0; e < WBG_GROUND_DOUBLES * B; e++) {
        const int f = (int)(e % WBG_GROUND_DOUBLES);
        const double x = ground[e];
        const std::string at = fn + ": instance " + std::to_string(e / WBG_GROUND_DOUBLES) + ", field " + std::to_string(f) + " (" + names[f] + "): ";
        if (f == 0) { if (!(std::isfinite(x) || (std::isinf(x) && x < 0.0))) return fail(at + "must be finite, or -inf for no ground"); }
        else if (f == 1 || f == 4) { if (!std::isfinite(x) || x <= 0.0) return fail(at + "must be finite and > 0"); }
        else if (f < 6) { if (!std::isfinite(x) || x < 0.0) return fail(at + "must be finite and >= 0"); }
        else if (x != 0.0 || std::signbit(x)) return fail(at + "must be 0");
    }
    Carve c;
    const auto a = c.add<double>(WBG_GROUND_DOUBLES * B);
    if (c.stage(h)) return -1;
    if (!h->d_ground) HIPCHK(hipMalloc(&h->d_ground, a.bytes()));
    std::memcpy(c.host(a), ground, a.bytes());
    HIPCHK(hipMemcpyAsync(h->d_ground, c.host(a), a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
static_assert(SRBM_TERRAIN_PATCHES == WBG_TERRAIN_PATCHES && SRBM_TERRAIN_DOUBLES == WBG_TERRAIN_DOUBLES, "include/srbm_rti.h states the terrain's sizes");
// the terrain of the ground (srbm_wb_terrain.hiph): validated, the unit normals formed here in double, the unused records empty
int srbm_wb_plant_set_terrain(srbm_batch* h, const double* terrain, int n_patches) {
    const std::string fn = "srbm_wb_plant_set_terrain";
    if (!h) return fail(fn + ": bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (!terrain) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_terrain) HIPCHK(hipFree(h->d_terrain));
        h->d_terrain = nullptr; h->terrain_patches = 0;
        return 0;
    }
    if (n_patches < 1 || n_patches > WBG_TERRAIN_PATCHES)
        return fail(fn + ": n_patches " + std::to_string(n_patches) + " is not in 1.." + std::to_string(WBG_TERRAIN_PATCHES));
    if (!h->d_ground) return fail(fn + ": a terrain is a setting of the ground, and the torque-driven plant has none (srbm_wb_plant_set_ground)");
    const size_t B = h->batch, P = n_patches;
    static const char* const names[WBG_TERRAIN_DOUBLES] = {"x_min", "x_max", "y_min", "y_max", "the height z0 at the world origin", "the slope gx", "the slope gy",
                                                           "the friction coefficient"};
    for (size_t e = 0; e < WBG_TERRAIN_DOUBLES * P * B; e++) {
        const int f = (int)(e % WBG_TERRAIN_DOUBLES);
        const double x = terrain[e];
        const std::string at = fn + ": instance " + std::to_string(e / (WBG_TERRAIN_DOUBLES * P)) + ", patch " + std::to_string(e / WBG_TERRAIN_DOUBLES % P) + ", field " +
                               std::to_string(f) + " (" + names[f] + "): ";
        if (std::isnan(x)) return fail(at + "is NaN");
        if (f >= 4 && !std::isfinite(x)) return fail(at + "must be finite");
        if (f == 7 && x < 0.0) return fail(at + "must be >= 0");
    }
    Carve c;
    const auto a = c.add<double>(WBT_INSTANCE_DOUBLES * B);
    if (c.stage(h)) return -1;
    double* rec = c.host(a);
    for (size_t b = 0; b < B; b++)
        for (size_t t = 0; t < WBG_TERRAIN_PATCHES; t++) {
            double* r = rec + (b * WBG_TERRAIN_PATCHES + t) * WBT_PATCH_DOUBLES;
            std::memset(r, 0, sizeof(double) * WBT_PATCH_DOUBLES);
            if (t >= P) { r[0] = 1.0; r[2] = 1.0; r[10] = 1.0; continue; }          // empty: x_min > x_max
            std::memcpy(r, terrain + (b * P + t) * WBG_TERRAIN_DOUBLES, sizeof(double) * WBG_TERRAIN_DOUBLES);
            const double gx = r[5], gy = r[6];
            const double gxx = gx * gx;
            const double gyy = gy * gy;
            const double s1 = 1.0 + gxx;
            const double s2 = s1 + gyy;
            const double s = std::sqrt(s2);
            r[8] = -gx / s; r[9] = -gy / s; r[10] = 1.0 / s;
        }
    if (!h->d_terrain) HIPCHK(hipMalloc(&h->d_terrain, a.bytes()));
    h->terrain_patches = n_patches;
    HIPCHK(hipMemcpyAsync(h->d_terrain, rec, a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_wb_plant_get_contact_state(srbm_batch* h, double* cs) {
    if (!h || !cs) return fail("srbm_wb_plant_get_contact_state: bad arguments");
    if (!h->d_wb) return fail(WB_NO_STATE);
    return fetch(h, {{cs, h->d_cs, sizeof(double) * WBG_CS_DOUBLES * (size_t)h->batch}});
}
int srbm_wb_plant_set_contact_state(srbm_batch* h, const double* cs) {
    const std::string fn = "srbm_wb_plant_set_contact_state";
    if (!h || !cs) return fail(fn + ": bad arguments");
    if (!h->d_wb) return fail(WB_NO_STATE);
    const size_t B = h->batch;
    for (size_t e = 0; e < WBG_CS_DOUBLES * B; e++) {
        const std::string at = fn + ": instance " + std::to_string(e / WBG_CS_DOUBLES) + ", foot " + std::to_string(e % WBG_CS_DOUBLES / 3) + ": ";
        if (e % 3 == 0) {
            if (!h->d_terrain) { if (cs[e] != 0.0 && cs[e] != 1.0) return fail(at + "in_contact must be 0 or 1"); }
            else if (!(cs[e] >= 0.0 && cs[e] <= (double)h->terrain_patches && cs[e] == std::floor(cs[e])))
                return fail(at + "in_contact must be 0, or 1 + the patch: an integer 0.." + std::to_string(h->terrain_patches) + " while a terrain is set");
        }
        else if (!std::isfinite(cs[e])) return fail(at + "the anchor is not finite");
    }
    HIPCHK(hipSetDevice(h->device));
    Carve c;
    const auto a = c.add<double>(WBG_CS_DOUBLES * B);
    if (c.stage(h)) return -1;
    std::memcpy(c.host(a), cs, a.bytes());
    HIPCHK(hipMemcpyAsync(h->d_cs, c.host(a), a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
static int ground_usable(srbm_batch* h, const char* fn) {
    if (fd_usable(h, fn)) return -1;
    if (!h->d_ground) return fail(std::string(fn) + ": the torque-driven plant has no ground (srbm_wb_plant_set_ground)");
    return 0;
}
int srbm_wb_ground_dynamics_dev(srbm_batch* h, const double* q_dev, const double* v_dev, const double* tau_dev, const double* cs_in_dev, double* sol_dev,
                                double* cs_out_dev, int* status_dev) {
    if (!h || !q_dev || !v_dev || !tau_dev || !cs_in_dev || !sol_dev || !cs_out_dev || !status_dev) return fail("srbm_wb_ground_dynamics: bad arguments");
    if (ground_usable(h, "srbm_wb_ground_dynamics") || use_batch(h)) return -1;
    int stride = 0;
    const SrbmBody* bodies = fd_bodies(h, &stride);
    if (joints_in_force(h) && terrain_in_force(h))
        hipLaunchKernelGGL((srbm_k_wb_ground_dynamics_joint<true>), dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, h->d_joints, h->d_ground,
                           h->d_terrain, q_dev, v_dev, tau_dev, cs_in_dev, sol_dev, cs_out_dev, status_dev);
    else if (joints_in_force(h))
        hipLaunchKernelGGL((srbm_k_wb_ground_dynamics_joint<false>), dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, h->d_joints, h->d_ground,
                           (const double*)nullptr, q_dev, v_dev, tau_dev, cs_in_dev, sol_dev, cs_out_dev, status_dev);
    else if (terrain_in_force(h))
        hipLaunchKernelGGL(srbm_k_wb_terrain_dynamics, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, h->d_ground, h->d_terrain, q_dev, v_dev,
                           tau_dev, cs_in_dev, sol_dev, cs_out_dev, status_dev);
    else
        hipLaunchKernelGGL(srbm_k_wb_ground_dynamics, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, bodies, stride, h->d_ground, q_dev, v_dev, tau_dev, cs_in_dev,
                           sol_dev, cs_out_dev, status_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_wb_ground_dynamics(srbm_batch* h, const double* q, const double* v, const double* tau, const double* cs_in, double* sol, double* cs_out, int* status) {
    if (!h || !q || !v || !tau || !cs_in || !sol || !cs_out) return fail("srbm_wb_ground_dynamics: bad arguments");
    if (ground_usable(h, "srbm_wb_ground_dynamics")) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    Carve c;                                          // in: q, v, tau, cs; out: sol, cs, status
    const auto iq = c.add<double>(19 * B), iv = c.add<double>(18 * B), it = c.add<double>(12 * B), ic = c.add<double>(WBG_CS_DOUBLES * B);
    const auto os = c.add<double>(WBC_NMAX * B), oc = c.add<double>(WBG_CS_DOUBLES * B);
    const auto ost = c.add<int>(B);
    if (c.stage(h)) return -1;
    memcpy(c.host(iq), q, iq.bytes());
    memcpy(c.host(iv), v, iv.bytes());
    memcpy(c.host(it), tau, it.bytes());
    memcpy(c.host(ic), cs_in, ic.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(iq), c.host(iq), Carve::span(iq, ic), hipMemcpyHostToDevice, h->stream));
    if (srbm_wb_ground_dynamics_dev(h, c.dev(iq), c.dev(iv), c.dev(it), c.dev(ic), c.dev(os), c.dev(oc), c.dev(ost))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(os), c.dev(os), Carve::span(os, ost), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(sol, c.host(os), os.bytes());
    memcpy(cs_out, c.host(oc), oc.bytes());
    if (status) memcpy(status, c.host(ost), ost.bytes());
    return 0;
}
int srbm_wb_ground_step_dev(srbm_batch* h, int tick, double tick_dt, double* q_dev, double* v_dev, double* cs_dev, const double* control_dev, const int* status_dev,
                            double* sol_dev) {
    if (!h || !q_dev || !v_dev || !cs_dev || !control_dev || !status_dev) return fail("srbm_wb_ground_step_dev: bad arguments");
    if (check_tick("srbm_wb_ground_step_dev", tick, tick_dt) || ground_usable(h, "srbm_wb_ground_step_dev")) return -1;
    if (!h->d_fd_act) return fail(std::string("srbm_wb_ground_step_dev: ") + FD_NO_ACTUATORS);
    if (use_batch(h)) return -1;
    return launch_wb_torque(h, tick, tick_dt, q_dev, v_dev, cs_dev, control_dev, nullptr, status_dev, nullptr, sol_dev, nullptr, nullptr);
}
// ---- the joint model of the torque-driven plant (srbm_wb_joints.hiph) ----
static_assert(SRBM_JOINT_DOUBLES == WBJ_JOINT_DOUBLES && SRBM_JOINT_STOP_DOUBLES == WBJ_STOP_DOUBLES && SRBM_JOINT_RECORD_DOUBLES == WBJ_RECORD_DOUBLES,
              "include/srbm_rti.h states the joint model's sizes");
static const char* const JOINTS_NOT_SET = "no joint model is set (srbm_wb_plant_set_joints)";
// the refusal of a joint model, naming instance, joint and field
static int check_joints(const std::string& fn, size_t B, const double* joints, const double* stops) {
    static const char* const names[WBJ_JOINT_DOUBLES] = {"the viscous damping b", "the armature I_a", "the dry friction f_c", "the stiction band v_s", "q_min", "q_max",
                                                         "the motor time constant T", "reserved"};
    for (size_t e = 0; e < WBJ_INSTANCE_DOUBLES * B; e++) {
        const int f = (int)(e % WBJ_JOINT_DOUBLES);
        const double x = joints[e];
        const double* c = joints + e - f;
        const std::string at = fn + ": instance " + std::to_string(e / WBJ_INSTANCE_DOUBLES) + ", joint " + std::to_string(e / WBJ_JOINT_DOUBLES % 12) + ", field " +
                               std::to_string(f) + " (" + names[f] + "): ";
        if (std::isnan(x)) return fail(at + "is NaN");
        if (f == WBJ_QMIN) { if (!(std::isfinite(x) || x < 0.0)) return fail(at + "must be finite or -inf"); }
        else if (f == WBJ_QMAX) {
            if (!(std::isfinite(x) || x > 0.0)) return fail(at + "must be finite or +inf");
            if (!(c[WBJ_QMIN] < x)) return fail(at + "q_min < q_max is required");
        }
        else if (f == WBJ_RESERVED) { if (x != 0.0 || std::signbit(x)) return fail(at + "must be 0"); }
        else if (!std::isfinite(x) || x < 0.0) return fail(at + "must be finite and >= 0");
        else if (f == WBJ_VS) {
            if (c[WBJ_FC] > 0.0 && !(x > 0.0)) return fail(at + "must be > 0 where the dry friction f_c is > 0");
            if (!(c[WBJ_FC] > 0.0) && x != 0.0) return fail(at + "must be 0 where the dry friction f_c is 0");
        }
    }
    for (size_t e = 0; e < WBJ_STOP_DOUBLES * B; e++) {
        const std::string at = fn + ": instance " + std::to_string(e / WBJ_STOP_DOUBLES) + ", stops, field " + std::to_string(e % WBJ_STOP_DOUBLES) +
                               (e % 2 ? " (the stop damping d_l): " : " (the stop stiffness k_l): ");
        if (!std::isfinite(stops[e])) return fail(at + "must be finite");
        if (e % 2 == 0 && !(stops[e] > 0.0)) return fail(at + "must be > 0");
        if (e % 2 == 1 && stops[e] < 0.0) return fail(at + "must be >= 0");
    }
    return 0;
}
int srbm_wb_plant_set_joints(srbm_batch* h, const double* joints, const double* stops) {
    const std::string fn = "srbm_wb_plant_set_joints";
    if (!h) return fail(fn + ": bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (!joints) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_joints) HIPCHK(hipFree(h->d_joints));
        h->d_joints = nullptr; h->joints.clear();
        return 0;
    }
    if (!stops) return fail(fn + ": bad arguments (joints without stops)");
    const size_t B = h->batch;
    if (check_joints(fn, B, joints, stops)) return -1;
    Carve c;
    const auto a = c.add<double>(JOINT_BUF_DOUBLES * B);
    if (c.stage(h)) return -1;
    if (!h->d_joints) HIPCHK(hipMalloc(&h->d_joints, a.bytes()));
    double* dst = c.host(a);
    std::memset(dst, 0, a.bytes());                                                  // the motor torques and the record at zero
    std::memcpy(dst, joints, sizeof(double) * WBJ_INSTANCE_DOUBLES * B);
    std::memcpy(dst + WBJ_INSTANCE_DOUBLES * B, stops, sizeof(double) * WBJ_STOP_DOUBLES * B);
    h->joints.assign(dst, dst + (WBJ_INSTANCE_DOUBLES + WBJ_STOP_DOUBLES) * B);
    HIPCHK(hipMemcpyAsync(h->d_joints, dst, a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_wb_plant_get_joints(srbm_batch* h, double* joints, double* stops) {
    if (!h || !joints || !stops) return fail("srbm_wb_plant_get_joints: bad arguments");
    if (!h->d_joints) return fail(std::string("srbm_wb_plant_get_joints: ") + JOINTS_NOT_SET);
    const size_t B = h->batch;
    std::memcpy(joints, h->joints.data(), sizeof(double) * WBJ_INSTANCE_DOUBLES * B);
    std::memcpy(stops, h->joints.data() + WBJ_INSTANCE_DOUBLES * B, sizeof(double) * WBJ_STOP_DOUBLES * B);
    return 0;
}
int srbm_wb_plant_get_joint_state(srbm_batch* h, double* js) {
    if (!h || !js) return fail("srbm_wb_plant_get_joint_state: bad arguments");
    if (!h->d_joints) return fail(std::string("srbm_wb_plant_get_joint_state: ") + JOINTS_NOT_SET);
    return fetch(h, {{js, joint_buf(h).js, sizeof(double) * 12 * (size_t)h->batch}});
}
int srbm_wb_plant_set_joint_state(srbm_batch* h, const double* js) {
    const std::string fn = "srbm_wb_plant_set_joint_state";
    if (!h || !js) return fail(fn + ": bad arguments");
    if (!h->d_joints) return fail(fn + ": " + JOINTS_NOT_SET);
    const size_t B = h->batch;
    for (size_t e = 0; e < 12 * B; e++)
        if (!std::isfinite(js[e])) return fail(fn + ": instance " + std::to_string(e / 12) + ", joint " + std::to_string(e % 12) + ": the motor torque is not finite");
    HIPCHK(hipSetDevice(h->device));
    Carve c;
    const auto a = c.add<double>(12 * B);
    if (c.stage(h)) return -1;
    std::memcpy(c.host(a), js, a.bytes());
    HIPCHK(hipMemcpyAsync(joint_buf(h).js, c.host(a), a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_wb_plant_get_joint_record(srbm_batch* h, double* jrec) {
    if (!h || !jrec) return fail("srbm_wb_plant_get_joint_record: bad arguments");
    if (!h->d_joints) return fail(std::string("srbm_wb_plant_get_joint_record: ") + JOINTS_NOT_SET);
    return fetch(h, {{jrec, joint_buf(h).jrec, sizeof(double) * WBJ_RECORD_DOUBLES * (size_t)h->batch}});
}
int srbm_joint_law_host(int batch, int substeps, double h, const double* joints, const double* stops, const double* cmd, const int* off, const double* q_j,
                        const double* v_j, double* js_inout, double* tau_out, double* jrec_inout) {
    const std::string fn = "srbm_joint_law_host";
    if (batch <= 0 || !joints || !stops || !cmd || !off || !q_j || !v_j || !js_inout || !tau_out) return fail(fn + ": bad arguments");
    if (substeps < 1 || !std::isfinite(h) || h <= 0.0) return fail(fn + ": substeps >= 1 and a finite h > 0 are required");
    const size_t B = batch;
    if (check_joints(fn, B, joints, stops)) return -1;
    const double hs = h / (double)substeps;
    for (size_t b = 0; b < B; b++) {
        double acc[3] = {0.0, 0.0, 0.0};
        int over = 0;
        unsigned mask = 0u;
        for (int s = 0; s < substeps; s++) {
            unsigned m = 0u;
            for (int j = 0; j < 12; j++) {
                const size_t at = ((size_t)s * B + b) * 12 + j;
                const double* c = joints + (b * 12 + j) * WBJ_JOINT_DOUBLES;
                double exc, fr, lag;
                tau_out[at] = srbm_joint_law(c, srbm_joint_alpha(c[WBJ_T], hs), stops[b * WBJ_STOP_DOUBLES], stops[b * WBJ_STOP_DOUBLES + 1], off[b] ? 0.0 : cmd[at],
                                             q_j[at], v_j[at], js_inout + b * 12 + j, &exc, &fr, &lag);
                acc[0] = fmax(acc[0], exc); acc[1] = fmax(acc[1], fr); acc[2] = fmax(acc[2], lag);
                m |= (exc > 0.0 ? 1u : 0u) << j;
            }
            over += m != 0u;
            mask |= m;
        }
        if (jrec_inout) srbm_joint_record_fold(jrec_inout + b * WBJ_RECORD_DOUBLES, substeps, over, acc[0], acc[1], acc[2], mask);
    }
    return 0;
}
// ---- the wrench schedule of the torque-driven plant (srbm_wb_wrench.hiph) ----
static_assert(SRBM_WRENCH_EVENTS == WBW_EVENTS && SRBM_WRENCH_DOUBLES == WBW_EVENT_DOUBLES && SRBM_WRENCH_RECORD_DOUBLES == WBW_RECORD_DOUBLES,
              "include/srbm_rti.h states the wrench schedule's sizes");
static const char* const WRENCHES_NOT_SET = "no wrench schedule is set (srbm_wb_plant_set_wrenches)";
// the refusal of a wrench schedule, naming instance, event and field
static int check_wrenches(const std::string& fn, size_t B, const double* wrenches, int n_events) {
    static const char* const names[WBW_EVENT_DOUBLES] = {"the start t0", "the duration d", "the body", "the frame", "the point r[0]", "the point r[1]", "the point r[2]",
                                                         "the force[0]", "the force[1]", "the force[2]", "the torque[0]", "the torque[1]", "the torque[2]", "reserved",
                                                         "reserved", "reserved"};
    if (n_events < 1 || n_events > WBW_EVENTS) return fail(fn + ": n_events " + std::to_string(n_events) + " (1.." + std::to_string(WBW_EVENTS) + " events per instance)");
    const size_t per = (size_t)n_events * WBW_EVENT_DOUBLES;
    for (size_t e = 0; e < per * B; e++) {
        const int f = (int)(e % WBW_EVENT_DOUBLES);
        const double x = wrenches[e];
        const std::string at = fn + ": instance " + std::to_string(e / per) + ", event " + std::to_string(e % per / WBW_EVENT_DOUBLES) + ", field " + std::to_string(f) +
                               " (" + names[f] + "): ";
        if (std::isnan(x)) return fail(at + "is NaN");
        if (f == WBW_D) { if (x < 0.0) return fail(at + "must be >= 0 or +inf (0: an empty slot)"); }
        else if (!std::isfinite(x)) return fail(at + "must be finite");
        else if (f == WBW_BODY) { if (!(x >= 0.0 && x <= 12.0 && x == std::floor(x))) return fail(at + "must be an integer 0..12 (0: the trunk, 1 + 3 leg + k)"); }
        else if (f == WBW_FRAME) { if (x != 0.0 && x != 1.0) return fail(at + "must be 0 (world axes) or 1 (the body's axes)"); }
        else if (f >= WBW_RESERVED) { if (x != 0.0 || std::signbit(x)) return fail(at + "must be 0"); }
    }
    return 0;
}
int srbm_wb_plant_set_wrenches(srbm_batch* h, const double* wrenches, int n_events) {
    const std::string fn = "srbm_wb_plant_set_wrenches";
    if (!h) return fail(fn + ": bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (!wrenches) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->d_wrench) HIPCHK(hipFree(h->d_wrench));
        h->d_wrench = nullptr; h->wrenches.clear(); h->wrench_events = 0;
        return 0;
    }
    const size_t B = h->batch;
    if (check_wrenches(fn, B, wrenches, n_events)) return -1;
    Carve c;
    const auto a = c.add<double>(WRENCH_BUF_DOUBLES * B);
    if (c.stage(h)) return -1;
    if (!h->d_wrench) HIPCHK(hipMalloc(&h->d_wrench, a.bytes()));
    double* dst = c.host(a);
    std::memset(dst, 0, a.bytes());                                                  // empty slots past n_events, the record at zero
    const size_t per = (size_t)n_events * WBW_EVENT_DOUBLES;
    for (size_t b = 0; b < B; b++) std::memcpy(dst + WBW_INSTANCE_DOUBLES * b, wrenches + per * b, sizeof(double) * per);
    h->wrenches.assign(wrenches, wrenches + per * B); h->wrench_events = n_events;
    HIPCHK(hipMemcpyAsync(h->d_wrench, dst, a.bytes(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_wb_plant_get_wrenches(srbm_batch* h, double* wrenches, int* n_events) {
    if (!h || !n_events) return fail("srbm_wb_plant_get_wrenches: bad arguments");
    if (!h->d_wrench) return fail(std::string("srbm_wb_plant_get_wrenches: ") + WRENCHES_NOT_SET);
    *n_events = h->wrench_events;
    if (wrenches) std::memcpy(wrenches, h->wrenches.data(), sizeof(double) * h->wrenches.size());
    return 0;
}
int srbm_wb_plant_get_wrench_record(srbm_batch* h, double* wrec) {
    if (!h || !wrec) return fail("srbm_wb_plant_get_wrench_record: bad arguments");
    if (!h->d_wrench) return fail(std::string("srbm_wb_plant_get_wrench_record: ") + WRENCHES_NOT_SET);
    return fetch(h, {{wrec, wrench_buf(h).wrec, sizeof(double) * WBW_RECORD_DOUBLES * (size_t)h->batch}});
}
int srbm_wb_wrench_force_dev(srbm_batch* h, const double* time_dev, const double* q_dev, double* Q_dev, int* mask_dev) {
    if (!h || !time_dev || !q_dev || !Q_dev || !mask_dev) return fail("srbm_wb_wrench_force: bad arguments");
    if (!h->d_wrench) return fail(std::string("srbm_wb_wrench_force: ") + WRENCHES_NOT_SET);
    if (need_legs(h) || use_batch(h)) return -1;
    hipLaunchKernelGGL(srbm_k_wb_wrench_force, dim3(h->batch), dim3(WBC_THREADS), 0, h->stream, h->dp, h->d_wrench, time_dev, q_dev, Q_dev, mask_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_wb_wrench_force(srbm_batch* h, const double* time, const double* q, double* Q_out, int* mask_out) {
    if (!h || !time || !q || !Q_out || !mask_out) return fail("srbm_wb_wrench_force: bad arguments");
    if (!h->d_wrench) return fail(std::string("srbm_wb_wrench_force: ") + WRENCHES_NOT_SET);
    if (need_legs(h)) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    Carve c;                                          // in: time, q; out: Q, mask
    const auto it = c.add<double>(B), iq = c.add<double>(19 * B), oq = c.add<double>(WBC_NV * B);
    const auto om = c.add<int>(B);
    if (c.stage(h)) return -1;
    memcpy(c.host(it), time, it.bytes());
    memcpy(c.host(iq), q, iq.bytes());
    HIPCHK(hipMemcpyAsync(c.dev(it), c.host(it), Carve::span(it, iq), hipMemcpyHostToDevice, h->stream));
    if (srbm_wb_wrench_force_dev(h, c.dev(it), c.dev(iq), c.dev(oq), c.dev(om))) return -1;
    HIPCHK(hipMemcpyAsync(c.host(oq), c.dev(oq), Carve::span(oq, om), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(Q_out, c.host(oq), oq.bytes());
    memcpy(mask_out, c.host(om), om.bytes());
    return 0;
}
int srbm_wrench_active_host(int n_events, const double* wrenches, int batch, int first_tick, int ticks, double tick_dt, int substeps, int* mask_out) {
    const std::string fn = "srbm_wrench_active_host";
    if (batch <= 0 || !wrenches || ticks < 0 || (ticks > 0 && !mask_out)) return fail(fn + ": bad arguments");
    if (substeps < 1) return fail(fn + ": substeps >= 1 is required");
    if (check_tick(fn.c_str(), first_tick, tick_dt)) return -1;
    const size_t B = batch;
    if (check_wrenches(fn, B, wrenches, n_events)) return -1;
    const double hs = tick_dt / (double)substeps;
    for (int k = 0; k < ticks; k++) {
        const double tk = (double)(first_tick + k) * tick_dt;
        for (int s = 0; s < substeps; s++) {
            const double ts = srbm_wrench_substep_time(tk, hs, s);
            for (size_t b = 0; b < B; b++) {
                int m = 0;
                for (int e = 0; e < n_events; e++) m |= (srbm_wrench_active(wrenches + (b * n_events + e) * WBW_EVENT_DOUBLES, ts) ? 1 : 0) << e;
                mask_out[((size_t)k * substeps + s) * B + b] = m;
            }
        }
    }
    return 0;
}
// ---- contact feedback from the ground (srbm_contact_feedback.hiph) ----
static int launch_contact_feedback(srbm_batch* h, const double* time, const double* cs) {
    const int tot = h->batch * SRBM_NEE;
    hipLaunchKernelGGL(srbm_k_contact_feedback, dim3((tot + 63) / 64), dim3(64), 0, h->stream, h->dp, h->insts, time, cs, h->d_fb);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_controller_set_contact_feedback(srbm_batch* h, int on) {
    if (!h) return fail("srbm_controller_set_contact_feedback: bad arguments");
    if (on != 0 && on != 1) return fail("srbm_controller_set_contact_feedback: on " + std::to_string(on) + " (0: off, 1: on)");
    h->contact_fb = on;
    return 0;
}
int srbm_controller_get_contact_feedback(srbm_batch* h, double* fb) {
    if (!h || !fb) return fail("srbm_controller_get_contact_feedback: bad arguments");
    if (!h->d_wb) return fail(WB_NO_STATE);
    return fetch(h, {{fb, h->d_fb, sizeof(double) * SRBM_FB_DOUBLES * (size_t)h->batch}});
}
int srbm_controller_contact_feedback_dev(srbm_batch* h, const double* time_dev, const double* cs_dev) {
    if (!h || !time_dev || !cs_dev) return fail("srbm_controller_contact_feedback_dev: bad arguments");
    if (!h->d_wb) return fail(WB_NO_STATE);
    if (use_batch(h)) return -1;
    return launch_contact_feedback(h, time_dev, cs_dev);
}
// ---- timed motion commands (srbm_command.hiph) ----
static_assert(SRBM_CMD_MAX_EVENTS == CMD_MAX_EVENTS && SRBM_CMD_EVENT_DOUBLES == CMD_EVENT_DOUBLES && SRBM_CMD_STATE_DOUBLES == CMD_STATE_DOUBLES &&
              SRBM_CMD_REC_DOUBLES == CMD_REC_DOUBLES, "include/srbm_rti.h states the command schedule's sizes");
int srbm_command_event_doubles(void) { return CMD_EVENT_DOUBLES; }
int srbm_command_record_doubles(void) { return CMD_REC_DOUBLES; }
static const char* const CMD_NOT_SET = "no command schedule is set (srbm_controller_set_commands)";
// the refusal of a command schedule, naming instance, event and field
static int check_commands(const std::string& fn, size_t B, const double* cmds, int n_events) {
    if (n_events < 0 || n_events > CMD_MAX_EVENTS) return fail(fn + ": n_events " + std::to_string(n_events) + " (0.." + std::to_string(CMD_MAX_EVENTS) + " events per instance)");
    if (n_events > 0 && !cmds) return fail(fn + ": bad arguments (NULL cmds)");
    const size_t per = (size_t)n_events * CMD_EVENT_DOUBLES;
    for (size_t e = 0; e < per * B; e++) {
        const int f = (int)(e % CMD_EVENT_DOUBLES), ev = (int)(e % per / CMD_EVENT_DOUBLES);
        const double x = cmds[e];
        const char* const name = f == CMD_T0 ? "the start t0" : f == CMD_FLAGS ? "the flags" : f == CMD_LEAD ? "the lead" : f == CMD_RESERVED ? "reserved" :
                                 f < CMD_RATE ? "des12" : "rate12";
        const std::string at = fn + ": instance " + std::to_string(e / per) + ", event " + std::to_string(ev) + ", field " + std::to_string(f) + " (" + name + "): ";
        if (!std::isfinite(x)) return fail(at + "must be finite");
        if (f == CMD_T0 && ev > 0 && !(x > cmds[e - CMD_EVENT_DOUBLES])) return fail(at + "must ascend strictly from event to event");
        if (f == CMD_FLAGS && x != 0.0 && x != 1.0) return fail(at + "must be 0 or 1 (bit 0: relative; no other bit)");
        if (f == CMD_LEAD && x < 0.0) return fail(at + "must be >= 0");
        if (f == CMD_RESERVED && (x != 0.0 || std::signbit(x))) return fail(at + "must be 0");
    }
    return 0;
}
static void command_reset_image(std::vector<double>& init, size_t B) {
    init.assign((CMD_STATE_DOUBLES + CMD_REC_DOUBLES) * B, 0.0);
    for (size_t b = 0; b < B; b++) { init[CMD_STATE_DOUBLES * b + CMD_S_INDEX] = -1.0; init[CMD_STATE_DOUBLES * B + CMD_REC_DOUBLES * b + CMD_R_INDEX] = -1.0; }
}
int srbm_controller_set_commands(srbm_batch* h, const double* cmds, int n_events) {
    const std::string fn = "srbm_controller_set_commands";
    if (!h) return fail(fn + ": bad arguments (NULL handle)");
    const size_t B = h->batch;
    if (check_commands(fn, B, cmds, n_events)) return -1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));          // (the buffer may be in use, the host image the source of a copy under way)
    if (h->d_cmd) HIPCHK(hipFree(h->d_cmd));
    h->d_cmd = nullptr; h->cmds.clear(); h->cmd_init.clear(); h->cmd_events = 0;
    params_changed(h);                                // the host's base costs are back on the device before anything else runs
    if (n_events == 0) return 0;
    const size_t per = (size_t)n_events * CMD_EVENT_DOUBLES;
    h->cmd_events = n_events;
    h->cmds.assign(cmds, cmds + per * B);
    command_reset_image(h->cmd_init, B);
    HIPCHK(hipMalloc(&h->d_cmd, sizeof(double) * cmd_buf_doubles(h)));
    const CmdBuf c = cmd_buf(h);
    HIPCHK(hipMemcpyAsync(c.cmds, h->cmds.data(), sizeof(double) * per * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(c.cstate, h->cmd_init.data(), sizeof(double) * h->cmd_init.size(), hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_controller_get_commands(srbm_batch* h, double* cmds, int* n_events) {
    if (!h || !n_events) return fail("srbm_controller_get_commands: bad arguments");
    *n_events = h->cmd_events;
    if (cmds && h->d_cmd) std::memcpy(cmds, h->cmds.data(), sizeof(double) * h->cmds.size());
    return 0;
}
int srbm_controller_get_command_state(srbm_batch* h, double* cstate) {
    if (!h || !cstate) return fail("srbm_controller_get_command_state: bad arguments");
    if (!h->d_cmd) return fail(std::string("srbm_controller_get_command_state: ") + CMD_NOT_SET);
    return fetch(h, {{cstate, cmd_buf(h).cstate, sizeof(double) * CMD_STATE_DOUBLES * (size_t)h->batch}});
}
int srbm_controller_set_command_state(srbm_batch* h, const double* cstate) {
    const std::string fn = "srbm_controller_set_command_state";
    if (!h || !cstate) return fail(fn + ": bad arguments");
    if (!h->d_cmd) return fail(fn + ": " + CMD_NOT_SET);
    for (size_t i = 0; i < CMD_STATE_DOUBLES * (size_t)h->batch; i++) {
        const double x = cstate[i];
        if (!std::isfinite(x)) return fail(fn + ": instance " + std::to_string(i / CMD_STATE_DOUBLES) + ", field " + std::to_string(i % CMD_STATE_DOUBLES) + ": must be finite");
        if (i % CMD_STATE_DOUBLES == CMD_S_INDEX && !(x >= -1.0 && x < (double)h->cmd_events && x == std::floor(x)))
            return fail(fn + ": instance " + std::to_string(i / CMD_STATE_DOUBLES) + ": the latched index must be an integer -1.." + std::to_string(h->cmd_events - 1));
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(cmd_buf(h).cstate, cstate, sizeof(double) * CMD_STATE_DOUBLES * (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    return srbm_synchronize(h);
}
int srbm_controller_get_command_record(srbm_batch* h, double* crec) {
    if (!h || !crec) return fail("srbm_controller_get_command_record: bad arguments");
    if (!h->d_cmd) return fail(std::string("srbm_controller_get_command_record: ") + CMD_NOT_SET);
    return fetch(h, {{crec, cmd_buf(h).crec, sizeof(double) * CMD_REC_DOUBLES * (size_t)h->batch}});
}
// w and Phi_w of the records on the device (no schedule is needed: without one they are the host's)
int srbm_controller_get_command_costs(srbm_batch* h, double* w, double* Phi_w) {
    if (!h || !w || !Phi_w) return fail("srbm_controller_get_command_costs: bad arguments");
    if (use_batch(h)) return -1;
    HIPCHK(hipStreamSynchronize(h->stream));
    const char* const base = reinterpret_cast<const char*>(h->dp);
    HIPCHK(hipMemcpy2D(w, sizeof(double) * 12, base + offsetof(SrbmParams, w), sizeof(SrbmParams), sizeof(double) * 12, h->batch, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(Phi_w, sizeof(double) * 12, base + offsetof(SrbmParams, Phi_w), sizeof(SrbmParams), sizeof(double) * 12, h->batch, hipMemcpyDeviceToHost));
    return 0;
}
// the command kernel before an MPC update at time[batch] on state[batch][13]; ls: nullptr, or the candidate batch of the gait handle that drives h
static int launch_command(srbm_batch* h, srbm_batch* ls, const double* time, const double* state) {
    const CmdBuf c = cmd_buf(h);
    hipLaunchKernelGGL(srbm_k_command, dim3(h->batch), dim3(CMD_THREADS), 0, h->stream, h->dp, ls ? ls->dp : nullptr, h->batch, c.cmds, h->cmd_events, time, state,
                       c.cstate, c.crec);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_controller_command_dev(srbm_batch* h, const double* time_dev, const double* state_dev) {
    if (!h || !time_dev || !state_dev) return fail("srbm_controller_command_dev: bad arguments");
    if (!h->d_cmd) return fail(std::string("srbm_controller_command_dev: ") + CMD_NOT_SET);
    if (use_batch(h)) return -1;
    return launch_command(h, nullptr, time_dev, state_dev);
}
int srbm_command_target_host(int n_events, const double* cmds, int batch, const double* Q144, const double* Phi144, int n_updates, const double* times,
                             const double* states13, double* cstate, double* des12, double* w12, double* Phi_w12, double* crec) {
    const std::string fn = "srbm_command_target_host";
    if (batch <= 0 || n_updates < 0 || !Q144 || !Phi144 || !cstate || !crec || (n_updates > 0 && (!times || !states13 || !des12 || !w12 || !Phi_w12)))
        return fail(fn + ": bad arguments");
    const size_t B = batch;
    if (check_commands(fn, B, cmds, n_events)) return -1;
    const double none = std::numeric_limits<double>::quiet_NaN();
    for (int u = 0; u < n_updates; u++)
        for (size_t b = 0; b < B; b++) {
            const size_t at = (size_t)u * B + b;
            double* const des = des12 + 12 * at;
            const double* const evs = cmds + b * n_events * CMD_EVENT_DOUBLES;
            const double t = times[at];
            const int index = srbm_cmd_in_force(evs, n_events, t);
            if (index < 0) {
                for (int i = 0; i < 12; i++) des[i] = w12[12 * at + i] = Phi_w12[12 * at + i] = none;
                continue;
            }
            const double* const ev = evs + index * CMD_EVENT_DOUBLES;
            const double x = states13[13 * at], y = states13[13 * at + 1];
            double ax, ay, unled[2];
            srbm_cmd_anchor(cstate + CMD_STATE_DOUBLES * b, index, x, y, &ax, &ay);
            srbm_cmd_target(ev, t, ax, ay, des, unled);
            for (int i = 0; i < 12; i++) {
                w12[12 * at + i] = srbm_cmd_cost_row(Q144 + 144 * b, i, des);
                Phi_w12[12 * at + i] = srbm_cmd_cost_row(Phi144 + 144 * b, i, des);
            }
            srbm_cmd_fold(ev, index, t, x, y, ax, ay, des, unled, cstate + CMD_STATE_DOUBLES * b, crec + CMD_REC_DOUBLES * b);
        }
    return 0;
}
// ---- MPC computation latency (srbm_mpc_latency.hiph) ----
static const char* const LAT_NOT_SET = "no latency is set (srbm_controller_set_latency)";
static int check_latency(const char* fn, int batch, const double* lat) {
    static const char* const field[SRBM_LAT_DOUBLES] = {"base", "per_iteration"};
    for (int i = 0; i < batch * SRBM_LAT_DOUBLES; i++)
        if (!std::isfinite(lat[i]) || lat[i] < 0.0) {
            char v[64]; std::snprintf(v, sizeof v, "%.17g", lat[i]);
            return fail(std::string(fn) + ": instance " + std::to_string(i / SRBM_LAT_DOUBLES) + ": " + field[i % SRBM_LAT_DOUBLES] + " is " + v +
                        " (a finite latency >= 0 in seconds is required)");
        }
    return 0;
}
int srbm_controller_set_latency(srbm_batch* h, const double* lat) {
    if (!h) return fail("srbm_controller_set_latency: bad arguments");
    if (lat && check_latency("srbm_controller_set_latency", h->batch, lat)) return -1;
    HIPCHK(hipSetDevice(h->device));
    const size_t B = h->batch;
    if (!lat) {
        HIPCHK(hipStreamSynchronize(h->stream));
        (void)hipFree(h->pub_insts); (void)hipFree(h->d_lat); (void)hipFree(h->d_pub);
        h->pub_insts = nullptr; h->d_lat = nullptr; h->d_pub = nullptr;
        h->lat.clear(); h->pub_init.clear();
        return 0;
    }
    if (!h->d_lat) HIPCHK(hipMalloc(&h->d_lat, sizeof(double) * SRBM_LAT_DOUBLES * B));
    if (!h->d_pub) HIPCHK(hipMalloc(&h->d_pub, sizeof(double) * SRBM_PUB_DOUBLES * B));
    if (!h->pub_insts) HIPCHK(hipMalloc(&h->pub_insts, sizeof(SrbmInst) * B));          // (last: it is what says that a latency is set)
    HIPCHK(hipStreamSynchronize(h->stream));                                              // (the host copies below may be the source of a copy under way)
    h->lat.assign(lat, lat + SRBM_LAT_DOUBLES * B);
    h->pub_init.assign(SRBM_PUB_DOUBLES * B, 0.0);
    for (size_t b = 0; b < B; b++) h->pub_init[b * SRBM_PUB_DOUBLES + 3] = -1.0;          // no publication yet
    HIPCHK(hipMemcpyAsync(h->d_lat, h->lat.data(), sizeof(double) * h->lat.size(), hipMemcpyHostToDevice, h->stream));
    if (latency_resync(h)) return -1;
    return srbm_synchronize(h);
}
int srbm_controller_get_latency_record(srbm_batch* h, double* pub) {
    if (!h || !pub) return fail("srbm_controller_get_latency_record: bad arguments");
    if (!h->pub_insts) return fail(std::string("srbm_controller_get_latency_record: ") + LAT_NOT_SET);
    return fetch(h, {{pub, h->d_pub, sizeof(double) * SRBM_PUB_DOUBLES * (size_t)h->batch}});
}
int srbm_controller_get_published(srbm_batch* h, int first, int count, srbm_trajectory* out) {
    if (!h || !out || first < 0 || count < 0 || first + count > h->batch) return fail("srbm_controller_get_published: bad arguments");
    if (!h->pub_insts) return fail(std::string("srbm_controller_get_published: ") + LAT_NOT_SET);
    std::vector<SrbmInst> v(count);
    if (fetch(h, {{v.data(), h->pub_insts + first, sizeof(SrbmInst) * (size_t)count}})) return -1;
    for (int i = 0; i < count; i++) inst_to_record(h->hp, v[i], out + i);
    return 0;
}
static int launch_publish(srbm_batch* h, const double* time, int update_number, double t_start, int force) {
    hipLaunchKernelGGL(srbm_k_mpc_publish, dim3(h->batch), dim3(SRBM_PUB_THREADS), 0, h->stream, h->insts, h->pub_insts, h->d_lat, time, h->d_pub, update_number,
                       t_start, force);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_controller_publish_dev(srbm_batch* h, const double* time_dev, int update_number, double t_start, int force) {
    const std::string fn = "srbm_controller_publish_dev: ";
    if (!h || !time_dev) return fail(fn + "bad arguments");
    if (!h->pub_insts) return fail(fn + LAT_NOT_SET);
    if (update_number < 0 || (force != 0 && force != 1) || !std::isfinite(t_start))
        return fail(fn + "update_number >= 0, a finite t_start and force 0 or 1 are required");
    if (use_batch(h)) return -1;
    return launch_publish(h, time_dev, update_number, t_start, force);
}
// The update started after tick k0 = u * ticks_per_update: t_start <- its start (an integer product, then one rounded product); -> the tick before
// whose targets kernel an instance with {base, per_iteration} whose solve took `iters` iterations is published; *overrun <- 1 if by force.
// The ticks k0 + 1 .. k0 + ticks_per_update as the kernel sees them, one after the other, through the rule functions the kernel calls.
static long long latency_publish_tick(long long u, int ticks_per_update, double tick_dt, double base, double per_iteration, int iters, int* overrun) {
    const long long k0 = u * ticks_per_update;
    const double t_start = (double)k0 * tick_dt;
    double L;
    const double due = srbm_latency_due(t_start, base, per_iteration, iters, &L);
    for (long long j = k0 + 1; ; j++) {
        const int what = srbm_latency_decide(0, 1, due, (double)j * tick_dt, j % ticks_per_update == 0);
        if (what) { if (overrun) *overrun = what == 2; return j; }
    }
}
int srbm_latency_publish_ticks_host(int batch, int first_tick, int ticks, int ticks_per_update, double tick_dt, const double* lat, const int* iters, int n_updates,
                                    int* publish_tick, int* overrun) {
    const char* fn = "srbm_latency_publish_ticks_host";
    if (batch <= 0 || !lat || !iters || n_updates < 0 || !publish_tick || !overrun) return fail(std::string(fn) + ": bad arguments");
    if (first_tick < 0 || ticks < 0 || ticks > INT_MAX - first_tick) return fail(std::string(fn) + ": first_tick >= 0 and ticks >= 0 are required");
    if (ticks_per_update < 1) return fail(std::string(fn) + ": ticks_per_update >= 1 is required");
    if (!std::isfinite(tick_dt) || tick_dt <= 0.0) return fail(std::string(fn) + ": a finite tick_dt > 0 is required");
    if (check_latency(fn, batch, lat)) return -1;
    for (int b = 0; b < batch; b++)
        for (int u = 1; u <= n_updates; u++) {
            const size_t at = (size_t)b * n_updates + (u - 1);
            if (iters[at] < 0) return fail(std::string(fn) + ": instance " + std::to_string(b) + ", update " + std::to_string(u) + ": a negative iteration count");
            int over = 0;
            const long long j = latency_publish_tick(u, ticks_per_update, tick_dt, lat[b * SRBM_LAT_DOUBLES], lat[b * SRBM_LAT_DOUBLES + 1], iters[at], &over);
            const bool inside = j >= first_tick && j < (long long)first_tick + ticks;
            publish_tick[at] = inside ? (int)j : -1;
            overrun[at] = inside ? over : 0;
        }
    return 0;
}
// srbm_controller_advance with a latency set: may an instance be published before the targets kernel of tick k?  need[j - k0 - 1] for the ticks
// k0 + 1 .. k0 + ticks_per_update of update u = k0 / ticks_per_update, from the rule itself: an instance is published no earlier than a solve of no
// iteration would be and no later than the longest solve would be (the due time grows with the count, rounding included) -- 2 (max_iter + 1) iterations,
// the two attempts of a solve with a lower start (srbm_k3_ipm.hiph), or the forced tick.  With per_iteration = 0 the two ticks are one.
// This is the tick for ANY instance pending for update u, whatever older update it holds; an instance whose tick lies before the first tick of a
// call (a rollout begun there) is due at that first tick, before which controller_advance always launches.
static void latency_ticks_needed(const srbm_batch* h, long long u, int ticks_per_update, double tick_dt, std::vector<char>& need) {
    need.assign(ticks_per_update, 0);
    const long long k0 = u * ticks_per_update;
    const int most = (int)std::min<long long>(INT_MAX, 2LL * ((long long)h->hp.max_iter + 1));
    for (int b = 0; b < h->batch; b++) {
        const double base = h->lat[b * SRBM_LAT_DOUBLES], per = h->lat[b * SRBM_LAT_DOUBLES + 1];
        const long long lo = latency_publish_tick(u, ticks_per_update, tick_dt, base, per, 0, nullptr);
        const long long hi = per > 0.0 ? latency_publish_tick(u, ticks_per_update, tick_dt, base, per, most, nullptr) : lo;
        for (long long j = lo; j <= hi; j++) need[j - k0 - 1] = 1;
    }
}
// ---- sensor model (srbm_sensors.hiph) ----
static const char* const SENS_NOT_SET = "no sensors are set (srbm_controller_set_sensors)";
static const char* const SENS_NO_STATE = "sensors are set but the plant's state is not (srbm_wb_plant_set_state): the sensor state starts from it";
static int check_sensors(const char* fn, int batch, const double* sens) {
    static const char* const field[SRBM_SENS_DOUBLES] = {"mocap_ticks", "mocap_delay", "sigma_p", "sigma_r", "velocity_source", "sigma_v", "sigma_w", "gyro_bias[0]",
                                                         "gyro_bias[1]", "gyro_bias[2]", "sigma_qj", "sigma_vj", "lpf_x_base", "lpf_x_joints", "reserved[14]",
                                                         "reserved[15]"};
    for (int i = 0; i < batch * SRBM_SENS_DOUBLES; i++) {
        const int f = i % SRBM_SENS_DOUBLES;
        const double x = sens[i];
        const char* need = nullptr;
        if (!std::isfinite(x)) need = "a finite value";
        else if (f == 0 && !(x == std::floor(x) && x >= 1.0 && x <= 64.0)) need = "an integer 1..64";
        else if (f == 1 && !(x == std::floor(x) && x >= 0.0 && x <= 3.0)) need = "an integer 0..3";
        else if (f == 4 && !(x == 0.0 || x == 1.0)) need = "0 (the plant's) or 1 (the finite difference)";
        else if (f >= 14 && x != 0.0) need = "0";
        else if (!(f >= 7 && f <= 9) && x < 0.0) need = "a value >= 0";
        if (need) {
            char v[64]; std::snprintf(v, sizeof v, "%.17g", x);
            return fail(std::string(fn) + ": instance " + std::to_string(i / SRBM_SENS_DOUBLES) + ": " + field[f] + " is " + v + " (" + need + " is required)");
        }
    }
    return 0;
}
int srbm_controller_set_sensors(srbm_batch* h, const double* sens, const long long* seed) {
    const char* fn = "srbm_controller_set_sensors";
    if (!h || (sens && !seed)) return fail(std::string(fn) + ": bad arguments");
    if (sens && check_sensors(fn, h->batch, sens)) return -1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t B = h->batch;
    if (!sens) {
        (void)hipFree(h->d_sens);
        h->d_sens = nullptr; h->sens_ready = false;
        h->sens.clear(); h->sens_seed.clear();
        return 0;
    }
    if (!h->d_sens) {
        HIPCHK(hipMalloc(&h->d_sens, sens_bytes(B)));
        HIPCHK(hipMemset(h->d_sens, 0, sens_bytes(B)));
        h->sens_ready = false;
    }
    h->sens.assign(sens, sens + SRBM_SENS_DOUBLES * B);
    h->sens_seed.resize(B);
    for (size_t b = 0; b < B; b++) h->sens_seed[b] = (unsigned long long)seed[b];
    std::vector<double> S(SRBM_SENS_DEV_DOUBLES * B);
    for (size_t b = 0; b < B; b++) srbm_sensor_device_record(sens + SRBM_SENS_DOUBLES * b, S.data() + SRBM_SENS_DEV_DOUBLES * b);
    const SensBuf s = sens_buf(h);
    HIPCHK(hipMemcpy(s.S, S.data(), sizeof(double) * S.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.seed, h->sens_seed.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice));
    if (!h->d_wb) return 0;          // (srbm_wb_plant_set_state will start the sensor state)
    // the sensor state starts from the plant's state as it is after the work queued so far
    std::vector<double> q(19 * B), v(18 * B);
    const WbBuf w = wb_buf(h);
    if (copy_each({{q.data(), w.q, sizeof(double) * q.size()}, {v.data(), w.v, sizeof(double) * v.size()}}, hipMemcpyDeviceToHost)) return -1;
    return sensors_reinit(h, q.data(), v.data());
}
int srbm_controller_get_sensors(srbm_batch* h, double* sens, long long* seed) {
    if (!h || !sens || !seed) return fail("srbm_controller_get_sensors: bad arguments");
    if (!h->d_sens) return fail(std::string("srbm_controller_get_sensors: ") + SENS_NOT_SET);
    std::memcpy(sens, h->sens.data(), sizeof(double) * h->sens.size());
    for (size_t b = 0; b < h->sens_seed.size(); b++) seed[b] = (long long)h->sens_seed[b];
    return 0;
}
int srbm_controller_get_sensor_state(srbm_batch* h, double* ms) {
    if (!h || !ms) return fail("srbm_controller_get_sensor_state: bad arguments");
    if (!h->d_sens) return fail(std::string("srbm_controller_get_sensor_state: ") + SENS_NOT_SET);
    if (!h->sens_ready) return fail(std::string("srbm_controller_get_sensor_state: ") + SENS_NO_STATE);
    return fetch(h, {{ms, sens_buf(h).ms, sizeof(double) * SRBM_SENS_STATE_DOUBLES * (size_t)h->batch}});
}
int srbm_controller_set_sensor_state(srbm_batch* h, const double* ms) {
    const std::string fn = "srbm_controller_set_sensor_state: ";
    if (!h || !ms) return fail(fn + "bad arguments");
    if (!h->d_sens) return fail(fn + SENS_NOT_SET);
    for (int b = 0; b < h->batch; b++) {
        const double n = ms[(size_t)b * SRBM_SENS_STATE_DOUBLES];
        if (!(std::isfinite(n) && n == std::floor(n) && n >= 0.0 && n <= 4503599627370496.0))
            return fail(fn + "instance " + std::to_string(b) + ": the sample count (entry 0) must be an integer 0 .. 2^52");
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(sens_buf(h).ms, ms, sizeof(double) * SRBM_SENS_STATE_DOUBLES * (size_t)h->batch, hipMemcpyHostToDevice));
    h->sens_ready = true;
    return 0;
}
int srbm_controller_get_sensor_record(srbm_batch* h, double* srec) {
    if (!h || !srec) return fail("srbm_controller_get_sensor_record: bad arguments");
    if (!h->d_sens) return fail(std::string("srbm_controller_get_sensor_record: ") + SENS_NOT_SET);
    return fetch(h, {{srec, sens_buf(h).srec, sizeof(double) * SRBM_SENS_RECORD_DOUBLES * (size_t)h->batch}});
}
int srbm_controller_get_measured(srbm_batch* h, double* q, double* v) {
    if (!h) return fail("srbm_controller_get_measured: bad arguments");
    if (!h->d_sens) return fail(std::string("srbm_controller_get_measured: ") + SENS_NOT_SET);
    const SensBuf s = sens_buf(h);
    return fetch(h, {{q, s.qm, sizeof(double) * 19 * (size_t)h->batch}, {v, s.vm, sizeof(double) * 18 * (size_t)h->batch}});
}
static int launch_measure(srbm_batch* h, int tick, double tick_dt, const double* q, const double* v, double* qm, double* vm) {
    const SensBuf s = sens_buf(h);
    hipLaunchKernelGGL(srbm_k_measure, dim3(h->batch), dim3(64), 0, h->stream, s.S, s.seed, tick, tick_dt, q, v, s.ms, s.srec, qm, vm);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_controller_measure_dev(srbm_batch* h, int tick, double tick_dt, const double* q_dev, const double* v_dev, double* qm_dev, double* vm_dev) {
    const std::string fn = "srbm_controller_measure_dev: ";
    if (!h || !q_dev || !v_dev || !qm_dev || !vm_dev) return fail(fn + "bad arguments");
    if (!h->d_sens) return fail(fn + SENS_NOT_SET);
    if (!h->sens_ready) return fail(fn + SENS_NO_STATE);
    if (q_dev == qm_dev || v_dev == vm_dev) return fail(fn + "the measurement must not be written over the true state");
    if (check_tick("srbm_controller_measure_dev", tick, tick_dt) || use_batch(h)) return -1;
    return launch_measure(h, tick, tick_dt, q_dev, v_dev, qm_dev, vm_dev);
}
int srbm_sensor_philox_host(const int* counter4, const int* key2, int* out4) {
    if (!counter4 || !key2 || !out4) return fail("srbm_sensor_philox_host: bad arguments");
    uint32_t c[4], k[2], o[4];
    std::memcpy(c, counter4, sizeof c); std::memcpy(k, key2, sizeof k);
    srbm_philox4x32_10(c, k, o);
    std::memcpy(out4, o, sizeof o);
    return 0;
}
int srbm_sensor_state_init_host(int batch, const double* q, const double* v, double* ms) {
    if (batch <= 0 || !q || !v || !ms) return fail("srbm_sensor_state_init_host: bad arguments");
    for (size_t b = 0; b < (size_t)batch; b++) srbm_sensor_state_init(q + 19 * b, v + 18 * b, ms + SRBM_SENS_STATE_DOUBLES * b);
    return 0;
}
int srbm_sensor_measure_host(int batch, int first_tick, int ticks, double tick_dt, const double* sens, const long long* seed, const double* q_true,
                             const double* v_true, double* ms_inout, double* srec_inout, double* qm_out, double* vm_out) {
    const char* fn = "srbm_sensor_measure_host";
    if (batch <= 0 || !sens || !seed || !q_true || !v_true || !ms_inout || !srec_inout || !qm_out || !vm_out) return fail(std::string(fn) + ": bad arguments");
    if (first_tick < 0 || ticks < 0 || ticks > INT_MAX - first_tick) return fail(std::string(fn) + ": first_tick >= 0 and ticks >= 0 are required");
    if (!std::isfinite(tick_dt) || tick_dt <= 0.0) return fail(std::string(fn) + ": a finite tick_dt > 0 is required");
    if (check_sensors(fn, batch, sens)) return -1;
    const size_t B = batch;
    std::vector<double> S(SRBM_SENS_DEV_DOUBLES * B);
    for (size_t b = 0; b < B; b++) srbm_sensor_device_record(sens + SRBM_SENS_DOUBLES * b, S.data() + SRBM_SENS_DEV_DOUBLES * b);
    for (int k = 0; k < ticks; k++)
        for (size_t b = 0; b < B; b++) {
            const size_t at = (size_t)k * B + b;
            srbm_sensor_measure_one(S.data() + SRBM_SENS_DEV_DOUBLES * b, (unsigned long long)seed[b], first_tick + k, tick_dt, q_true + 19 * at, v_true + 18 * at,
                                    ms_inout + SRBM_SENS_STATE_DOUBLES * b, srec_inout + SRBM_SENS_RECORD_DOUBLES * b, qm_out + 19 * at, vm_out + 18 * at);
        }
    return 0;
}
// MPCController::MPCUpdate's branch on the run number (mpc_controller.cpp:324-346) as srbm_gait_rti_advance has it, on the state, time and ee of
// the tick (device arrays of the batch), with the record of the run where a step log is enabled
static int gait_update(srbm_gait* g, int run, int F, const double* state, const double* time, const double* ee) {
    srbm_batch* h = g->h;
    const size_t B = h->batch;
    if (run % F != 0 && (run + 1) % F != 0) {
        if (srbm_get_real_time_update_dev(h, state, time, ee)) return -1;
        launch_gait_ready(g, 0);
        HIPCHK(hipGetLastError());
        return 0;
    }
    HIPCHK(hipMemcpyAsync(h->d_state, state, sizeof(double) * 13 * B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ee, ee, sizeof(double) * 12 * B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_time, time, sizeof(double) * B, hipMemcpyDeviceToDevice, h->stream));
    if (run % F == 0) {
        // instances without a ready gradient get the plain update through the same 10-candidate batch (zero step)
        if (line_search_core(g, true) || log_gait_step(g, SRBM_GAIT_RUN_LINE_SEARCH)) return -1;          // (logged before the flag is reset: it tells who searched)
        launch_gait_ready(g, 0);
    } else {
        // the solve the gradient differentiates: to the gap criterion whatever the batch's step rule says (srbm_gait_rti_advance)
        if (launch_step(h, true) || gait_opt_core(g) || log_gait_step(g, SRBM_GAIT_RUN_GRADIENT)) return -1;
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// The loop of srbm_controller_advance and srbm_gait_controller_advance.  g: nullptr, or the gait handle whose batch is h: the update after tick k
// is then run k / ticks_per_update of the branch of srbm_gait_rti_advance.
static int controller_advance(const std::string& fn, srbm_batch* h, srbm_gait* g, int first_tick, int ticks, int ticks_per_update, double tick_dt, int gait_opt_freq) {
    if (!h->d_wb) return fail(fn + ": the whole-body plant state has not been set (srbm_wb_plant_set_state)");
    if (tick_usable(h)) return -1;
    if (h->fd_kind == 1 && !h->d_fd_act) return fail(fn + ": " + FD_NO_ACTUATORS);
    if (h->d_sens && !h->sens_ready) return fail(fn + ": " + SENS_NO_STATE);
    if (h->contact_fb && !(h->fd_kind == 1 && h->d_ground))
        return fail(fn + ": contact feedback is on (srbm_controller_set_contact_feedback) and needs the torque-driven plant with a ground "
                    "(srbm_wb_plant_set_kind 1, srbm_wb_plant_set_ground): without a ground nothing measures a contact");
    if (first_tick < 0 || ticks < 0 || ticks > INT_MAX - first_tick) return fail(fn + ": first_tick >= 0 and ticks >= 0 are required");
    if (ticks_per_update < 1) return fail(fn + ": ticks_per_update >= 1 is required");
    if (!std::isfinite(tick_dt) || tick_dt <= 0.0) return fail(fn + ": a finite tick_dt > 0 is required");
    const double period = ticks_per_update * tick_dt, horizon = h->hp.N * h->hp.dt;
    if (!(period < horizon)) {
        char v[64]; std::snprintf(v, sizeof v, "%.17g", period);
        return fail(fn + ": the MPC period ticks_per_update * tick_dt is " + v + ": a period below num_nodes * dt = " + std::to_string(horizon) +
                    " is required (beyond it the ticks would read past the trajectory)");
    }
    // with a latency set a tick can read a trajectory that started up to two periods ago
    if (h->pub_insts && !(2.0 * period < horizon)) {
        char v[64]; std::snprintf(v, sizeof v, "%.17g", 2.0 * period);
        return fail(fn + ": a latency is set (srbm_controller_set_latency) and twice the MPC period, 2 * ticks_per_update * tick_dt, is " + v +
                    ": below num_nodes * dt = " + std::to_string(horizon) + " is required (a tick can read a trajectory up to two periods old)");
    }
    // an MPC update follows tick k > 0 with k % ticks_per_update == 0
    auto updates_before = [&](long long k) { return k <= 0 ? 0LL : (k - 1) / ticks_per_update; };          // such k in [0, k)
    const int updates = (int)(updates_before((long long)first_tick + ticks) - updates_before(first_tick));
    if (h->d_tlog && ticks > h->tlog_cap - h->tlog_used)
        return fail(fn + ": the tick log has room for " + std::to_string(h->tlog_cap - h->tlog_used) + " more ticks (" + std::to_string(h->tlog_used) + " of " +
                    std::to_string(h->tlog_cap) + " logged), the call asks for " + std::to_string(ticks) + " (srbm_tick_log_reset, or srbm_tick_log_enable with more ticks)");
    if (log_room(h, fn.c_str(), updates)) return -1;
    if (use_batch(h)) return -1;
    if (ticks == 0) return 0;
    const size_t B = h->batch;
    const WbBuf w = wb_buf(h);
    hipLaunchKernelGGL(srbm_k_wb_tick_time, dim3((h->batch + 63) / 64), dim3(64), 0, h->stream, w.time + (first_tick & 1) * B, h->batch, first_tick, tick_dt);
    const SensBuf sb = h->d_sens ? sens_buf(h) : SensBuf{};
    std::vector<char> pub_need;          // with a latency set: the ticks of update pub_need_u before which the publish kernel is launched
    long long pub_need_u = 0;
    for (int k = first_tick; k < first_tick + ticks; k++) {
        double* const time = w.time + (k & 1) * B;
        const bool update = k > 0 && k % ticks_per_update == 0;
        // the last update started before tick k is due, or forced, for some instance: its trajectories are published before the tick reads them
        const long long e = updates_before(k);
        if (h->pub_insts && e >= 1) {
            if (e != pub_need_u) { latency_ticks_needed(h, e, ticks_per_update, tick_dt, pub_need); pub_need_u = e; }
            // (... and before the first tick of every call: pub_need holds for a rollout that has run since update e started.  One begun here on a
            // state just set has update 0 in force, and whatever the rule would have published before this tick is due now.  In a continued rollout
            // that launch finds nobody both pending and due and touches nothing.)
            if ((k == first_tick || pub_need[k - e * ticks_per_update - 1]) &&
                launch_publish(h, time, (int)e, (double)(e * ticks_per_update) * tick_dt, update ? 1 : 0)) return -1;
        }
        // with sensors set the tick reads the measurement of (q, v), made now; the plant, the push, the ground and the tick-log head keep the truth
        if (h->d_sens && launch_measure(h, k, tick_dt, w.q, w.v, sb.qm, sb.vm)) return -1;
        if (srbm_control_tick_dev(h, h->d_sens ? sb.qm : w.q, h->d_sens ? sb.vm : w.v, time, w.control, w.sol, w.status, nullptr, nullptr, w.contact, w.state,
                                  w.ee)) return -1;
        // mpc_controller.cpp:322: the contacts measured at t_k -- the ground's state after tick k - 1 -- re-time the plan the update starts from
        if (update && h->contact_fb && launch_contact_feedback(h, time, h->d_cs)) return -1;
        // the command in force at t_k on the tick's reconstructed state becomes the costs of the update (srbm_command.hiph); the candidates' records
        // are brought up to date first, so that the line search uploads nothing over what the kernel wrote
        if (update && h->d_cmd && ((g && candidate_records_current(g)) || launch_command(h, g ? g->ls : nullptr, time, w.state))) return -1;
        const SrbmTickLogArgs lg{h->d_tlog ? h->d_tlog + (size_t)h->tlog_used * B * SRBM_TICK_LOG_DOUBLES : nullptr, w.control, w.ee, w.contact, update ? 1 : 0};
        if (h->fd_kind == 1) {
            if (launch_wb_torque(h, k, tick_dt, w.q, w.v, h->d_ground ? h->d_cs : nullptr, w.control, w.contact, w.status, w.sol, nullptr, w.time + ((k + 1) & 1) * B,
                                 h->d_tlog ? &lg : nullptr)) return -1;
        } else if (launch_wb_plant(h, k, tick_dt, w.q, w.v, w.sol, w.status, w.time + ((k + 1) & 1) * B, h->d_tlog ? &lg : nullptr)) return -1;
        if (h->d_tlog) h->tlog_used++;
        // the hand-off of mpc_controller.cpp:142-156: the state and foot positions of THIS tick to the solve, the new trajectories in force from tick k + 1
        if (update && !g && srbm_get_real_time_update_dev(h, w.state, time, w.ee)) return -1;
        if (update && g && gait_update(g, k / ticks_per_update, gait_opt_freq, w.state, time, w.ee)) return -1;
    }
    return 0;
}
int srbm_controller_advance(srbm_batch* h, int first_tick, int ticks, int ticks_per_update, double tick_dt) {
    const std::string fn = "srbm_controller_advance";
    if (!h) return fail(fn + ": bad arguments (NULL handle)");
    return controller_advance(fn, h, nullptr, first_tick, ticks, ticks_per_update, tick_dt, 0);
}
int srbm_gait_controller_advance(srbm_gait* g, int first_tick, int ticks, int ticks_per_update, double tick_dt, int gait_opt_freq) {
    const std::string fn = "srbm_gait_controller_advance";
    if (!g) return fail(fn + ": bad arguments (NULL handle)");
    if (gait_opt_freq <= 0) return fail(fn + ": gait_opt_freq > 0 is required");
    return controller_advance(fn, g->h, g, first_tick, ticks, ticks_per_update, tick_dt, gait_opt_freq);
}
// ---- the tick log (include/srbm_rti.h; the record is written by srbm_k_wb_plant_step<true>) ----
int srbm_tick_log_record_doubles(void) { return SRBM_TICK_LOG_DOUBLES; }
int srbm_tick_log_enable(srbm_batch* h, int max_ticks) {
    if (!h || max_ticks < 0) return fail("srbm_tick_log_enable: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_tlog) HIPCHK(hipFree(h->d_tlog));
    h->d_tlog = nullptr; h->tlog_cap = 0; h->tlog_used = 0;
    if (max_ticks == 0) return 0;
    HIPCHK(hipMalloc(&h->d_tlog, sizeof(double) * SRBM_TICK_LOG_DOUBLES * (size_t)h->batch * (size_t)max_ticks));
    h->tlog_cap = max_ticks;
    return 0;
}
int srbm_tick_log_reset(srbm_batch* h) {
    if (!h) return fail("srbm_tick_log_reset: bad arguments");
    h->tlog_used = 0;
    return 0;
}
int srbm_tick_log_count(srbm_batch* h, int* ticks_logged) {
    if (!h || !ticks_logged) return fail("srbm_tick_log_count: bad arguments");
    *ticks_logged = h->tlog_used;
    return 0;
}
static int tick_log_range(const srbm_batch* h, const char* fn, int first_slot, int count, const void* out, const double** src, size_t* bytes) {
    if (!h || !out) return fail(std::string(fn) + ": bad arguments");
    if (!h->d_tlog) return fail(std::string(fn) + ": no tick log is enabled on this batch (srbm_tick_log_enable)");
    if (first_slot < 0 || count < 0 || first_slot > h->tlog_used || count > h->tlog_used - first_slot)
        return fail(std::string(fn) + ": slots [" + std::to_string(first_slot) + ", " + std::to_string((long long)first_slot + count) + ") are outside the " +
                    std::to_string(h->tlog_used) + " ticks logged");
    const size_t rec = (size_t)SRBM_TICK_LOG_DOUBLES * h->batch;
    *src = h->d_tlog + rec * first_slot;
    *bytes = sizeof(double) * rec * count;
    return 0;
}
int srbm_tick_log_get(srbm_batch* h, int first_slot, int count, double* out) {
    const double* src = nullptr; size_t bytes = 0;
    if (tick_log_range(h, "srbm_tick_log_get", first_slot, count, out, &src, &bytes)) return -1;
    if (bytes == 0) return 0;
    return fetch(h, {{out, src, bytes}});
}
int srbm_tick_log_copy_dev(srbm_batch* h, int first_slot, int count, double* out_dev) {
    const double* src = nullptr; size_t bytes = 0;
    if (tick_log_range(h, "srbm_tick_log_copy_dev", first_slot, count, out_dev, &src, &bytes)) return -1;
    if (bytes == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out_dev, src, bytes, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// ---- tick summaries (include/srbm_rti.h; csrc/srbm_tick_summary.hiph): the entries of the rollout summaries, on the tick log ----
int srbm_tick_summary_doubles(void) { return SRBM_TICK_SUMMARY_DOUBLES; }
static_assert(SRBM_TICK_CRITERIA_DOUBLES == SRBM_ROLLOUT_CRITERIA_DOUBLES, "rollout_check_criteria checks both sets: finite, entries 6 and 7 zero");
static int tick_summary_enabled(const srbm_batch* h, const char* fn) {
    if (!h) return fail(std::string(fn) + ": bad arguments");
    if (!h->d_tsum) return fail(std::string(fn) + ": no tick summary is enabled on this batch (srbm_tick_summary_enable)");
    return 0;
}
static int tick_slots_outside(const char* fn, int first_slot, int count, int slots, const char* what) {
    if (first_slot < 0 || count < 0 || first_slot > slots || count > slots - first_slot)
        return fail(std::string(fn) + ": slots [" + std::to_string(first_slot) + ", " + std::to_string((long long)first_slot + count) + ") are outside the " +
                    std::to_string(slots) + what);
    return 0;
}
int srbm_tick_summary_reset(srbm_batch* h) {
    if (tick_summary_enabled(h, "srbm_tick_summary_reset")) return -1;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_tsum, h->tsum_init.data(), sizeof(double) * h->tsum_init.size(), hipMemcpyHostToDevice, h->stream));
    return 0;
}
int srbm_tick_summary_enable(srbm_batch* h, const double* criteria, const double* ref) {
    if (!h) return fail("srbm_tick_summary_enable: bad arguments");
    if (criteria) {
        if (!ref) return fail("srbm_tick_summary_enable: criteria without references (ref[batch][6])");
        if (rollout_check_criteria("srbm_tick_summary_enable", criteria)) return -1;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_tsum) HIPCHK(hipFree(h->d_tsum));
    h->d_tsum = nullptr;
    if (h->d_tsum_ref) HIPCHK(hipFree(h->d_tsum_ref));
    h->d_tsum_ref = nullptr;
    if (!criteria) return 0;
    const size_t B = h->batch;
    std::memcpy(h->tsum_crit.c, criteria, sizeof(h->tsum_crit.c));
    h->tsum_init.resize(B * SRBM_TICK_SUMMARY_DOUBLES);
    for (size_t b = 0; b < B; b++) srbm_tick_summary_init(h->tsum_init.data() + b * SRBM_TICK_SUMMARY_DOUBLES);
    HIPCHK(hipMalloc(&h->d_tsum_ref, sizeof(double) * SRBM_TICK_REF_DOUBLES * B));
    HIPCHK(hipMemcpy(h->d_tsum_ref, ref, sizeof(double) * SRBM_TICK_REF_DOUBLES * B, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&h->d_tsum, sizeof(double) * SRBM_TICK_SUMMARY_DOUBLES * B));
    return srbm_tick_summary_reset(h);
}
// the fold kernel on log[slots][batch][64] of the batch's device: the range is checked by the callers
static int tick_fold_launch(srbm_batch* h, const double* log, int first_slot, int count) {
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(srbm_k_tick_fold, dim3(h->batch), dim3(64), 0, h->stream, log, h->batch, first_slot, count, h->tsum_crit, h->d_tsum_ref, h->d_tsum);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_tick_summary_fold(srbm_batch* h, int first_slot, int count) {
    if (!h) return fail("srbm_tick_summary_fold: bad arguments");
    if (!h->d_tlog) return fail("srbm_tick_summary_fold: no tick log is enabled on this batch (srbm_tick_log_enable)");
    if (tick_summary_enabled(h, "srbm_tick_summary_fold")) return -1;
    if (tick_slots_outside("srbm_tick_summary_fold", first_slot, count, h->tlog_used, " ticks logged")) return -1;
    return tick_fold_launch(h, h->d_tlog, first_slot, count);
}
int srbm_tick_summary_fold_dev(srbm_batch* h, const double* log_dev, int slots, int first_slot, int count) {
    if (!h || !log_dev || slots < 0) return fail("srbm_tick_summary_fold_dev: bad arguments");
    if (tick_summary_enabled(h, "srbm_tick_summary_fold_dev")) return -1;
    if (tick_slots_outside("srbm_tick_summary_fold_dev", first_slot, count, slots, " slots of the log")) return -1;
    return tick_fold_launch(h, log_dev, first_slot, count);
}
int srbm_tick_summary_get(srbm_batch* h, int first, int count, double* out) {
    if (tick_summary_enabled(h, "srbm_tick_summary_get")) return -1;
    if (!out) return fail("srbm_tick_summary_get: bad arguments");
    if (first < 0 || count < 0 || first > h->batch || count > h->batch - first)
        return fail("srbm_tick_summary_get: instances [" + std::to_string(first) + ", " + std::to_string((long long)first + count) + ") are outside the batch of " +
                    std::to_string(h->batch));
    if (count == 0) return 0;
    return fetch(h, {{out, h->d_tsum + (size_t)first * SRBM_TICK_SUMMARY_DOUBLES, sizeof(double) * SRBM_TICK_SUMMARY_DOUBLES * count}});
}
int srbm_tick_summary_copy_dev(srbm_batch* h, double* out_dev) {
    if (tick_summary_enabled(h, "srbm_tick_summary_copy_dev")) return -1;
    if (!out_dev) return fail("srbm_tick_summary_copy_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out_dev, h->d_tsum, sizeof(double) * SRBM_TICK_SUMMARY_DOUBLES * (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
int srbm_tick_study_dev(srbm_batch* h, const double* summaries_dev, int instances, double* study_dev) {
    if (!h || !summaries_dev || !study_dev || instances < 0) return fail("srbm_tick_study_dev: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(srbm_k_tick_study, dim3(1), dim3(64), 0, h->stream, summaries_dev, instances, study_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int srbm_tick_study(srbm_batch* h, double* study) {
    if (tick_summary_enabled(h, "srbm_tick_study")) return -1;
    if (!study) return fail("srbm_tick_study: bad arguments");
    void* d = nullptr;
    if (batch_scratch(h, sizeof(double) * SRBM_TICK_STUDY_DOUBLES, &d)) return -1;
    if (srbm_tick_study_dev(h, h->d_tsum, h->batch, static_cast<double*>(d))) return -1;
    return fetch(h, {{study, d, sizeof(double) * SRBM_TICK_STUDY_DOUBLES}});
}
int srbm_tick_summary_allgather_dev(srbm_batch* h, ncclComm_t comm, double* out_dev) {
    if (tick_summary_enabled(h, "srbm_tick_summary_allgather_dev")) return -1;
    const size_t count = (size_t)h->batch * SRBM_TICK_SUMMARY_DOUBLES;
    double* mine = nullptr;
    if (allgather_slot("srbm_tick_summary_allgather_dev", h, comm, out_dev, count, &mine)) return -1;
    if (srbm_tick_summary_copy_dev(h, mine)) return -1;
    return allgather_run(h, comm, mine, out_dev, count);
}
// the same fold and the same reduction on the host: no GPU, no batch
int srbm_tick_fold_host(const double* log, int slots, int batch, int first_slot, int count, const double* criteria, const double* ref, double* summaries) {
    if (!log || !criteria || !ref || !summaries || slots < 0 || batch < 1) return fail("srbm_tick_fold_host: bad arguments");
    if (rollout_check_criteria("srbm_tick_fold_host", criteria)) return -1;
    if (tick_slots_outside("srbm_tick_fold_host", first_slot, count, slots, " slots of the log")) return -1;
    for (int b = 0; b < batch; b++)
        for (int s = first_slot; s < first_slot + count; s++)
            srbm_tick_fold_record(summaries + (size_t)b * SRBM_TICK_SUMMARY_DOUBLES, log + ((size_t)s * batch + b) * SRBM_TICK_LOG_DOUBLES, criteria,
                                  ref + (size_t)b * SRBM_TICK_REF_DOUBLES);
    return 0;
}
int srbm_tick_study_host(const double* summaries, int instances, double* study) {
    if (!summaries || !study || instances < 0) return fail("srbm_tick_study_host: bad arguments");
    double U[SRBM_TICK_STUDY_DOUBLES];
    srbm_tick_study_init(U);
    for (int i = 0; i < instances; i++) srbm_tick_study_add(U, summaries + (size_t)i * SRBM_TICK_SUMMARY_DOUBLES);
    std::memcpy(study, U, sizeof(U));
    return 0;
}

}  // extern "C"
