// C-ABI of include/tcv.h: the device-resident batch at work -- ceres::Solve (tcv_batch_solve), the marginalisation's launch, the wait for
// what is in flight with the streams' bookkeeping (tcv_batch.h BatchFlight), and the getters that describe the launch: cooperative mode,
// profile, layout, plan statistics.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "tcv_host.h"

using namespace tcv;

extern "C" int tcv_launch_solve(const tcv::SolveArgs *args, int grid, int nthreads, size_t lds_bytes, void *stream);
extern "C" int tcv_solve_scratch_doubles(void);

extern "C" void tcv_solver_options_default(tcv_solver_options *o) {
    if (!o) return;
    o->max_num_iterations = 8;
    o->max_solver_time_in_seconds = 0.0;
    o->fixed_iterations = 0;
    o->workgroups_per_window = 0;
    o->use_mfma = 1;
    o->threads_per_window = 256;
    o->record_first_step = 0;
}

int tcv::BatchFlight::enter(hipStream_t st) {
    if (wait_inflight) HIPCHK(hipStreamWaitEvent(st, ev_inflight, 0));      // (the stream that work ran on may be gone: its event orders the new call)
    else if (pending && last_stream != st) {
        if (!ev_order) HIPCHK(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev_order, last_stream));
        HIPCHK(hipStreamWaitEvent(st, ev_order, 0));
    }
    if (std::find(streams.begin(), streams.end(), st) == streams.end()) streams.push_back(st);
    last_stream = st; pending = true;
    return TCV_OK;
}
hipError_t tcv::BatchFlight::wait_all() {
    hipError_t e = wait_inflight ? hipEventSynchronize(ev_inflight) : hipSuccess;
    for (hipStream_t st : streams) { const hipError_t es = st ? hipStreamSynchronize(st) : hipDeviceSynchronize(); if (e == hipSuccess) e = es; }
    if (e == hipSuccess) { wait_inflight = false; streams.clear(); pending = false; }
    return e;
}
hipError_t tcv::BatchFlight::track_by_event() {
    hipError_t e = hipSuccess;
    if (!ev_inflight) e = hipEventCreateWithFlags(&ev_inflight, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev_inflight, last_stream);
    if (e == hipSuccess) { streams.clear(); wait_inflight = true; }
    return e;
}

static int wall_clock_khz() {
    int dev = 0, khz = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;      // 100 MHz on CDNA
    return khz;
}
extern "C" int tcv_batch_solve(tcv_batch *b, const tcv_solver_options *o, void *hip_stream) {
    if (!b || !o) return TCV_ERR_INVALID;
    const hipStream_t st = tcv::resolve_stream(hip_stream);
    SolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->mem.d_win; a.plans = b->mem.d_plans; a.plan_base = b->mem.d_plan_base; a.ipool = b->mem.d_ipool; a.dpool = b->mem.d_dpool;
    a.state_out = b->mem.d_state; a.summary = b->mem.d_summary; a.first_delta = o->record_first_step ? b->mem.d_delta : nullptr;
    a.scratch = b->mem.d_scratch;
    a.prof = b->mem.d_prof;
    a.nwin = b->in.n; a.state_stride = b->in.state_stride; a.delta_stride = b->in.delta_stride; a.scratch_stride = tcv_solve_scratch_doubles() + b->shape.hcl_cap;
    a.max_iterations = o->max_num_iterations; a.fixed_iterations = o->fixed_iterations; a.use_mfma = o->use_mfma;
    a.chain = b->shape.chain ? 1 : 0; a.chain_td = b->shape.chain_td ? 1 : 0;
    a.imublk = b->mem.d_imublk; a.spill = b->mem.d_spill; a.spill_stride = b->shape.spill_stride;
    a.max_ticks = 0;
    a.sqrt_out = b->mem.d_sqrt_out;
    // (a batch with a relocalisation window never fuses: double2vector's tail needs the un-fixed pose 0, tcv_relo.hip; the stand-alone kernel gives the same bits)
    a.gauge_fix = b->last.fuse_gauge && !tcv_relo_of(b) ? 1 : 0;
    // cooperative plans also run on the single-workgroup kernel (workgroups_per_window = 1): same chunks, same additions, same bits
    bool coop = b->coop.h > 0 && o->workgroups_per_window != 1;
    if (coop && b->claim.total == 0)      // (a claim still held: the previous cooperative solve of this batch, same stream order, same rotation)
        if (!coop_admit(b->shape.dev, b->shape.n_cu, b->coop.groups, 1 + b->coop.h, &b->claim)) coop = false;      // the XCDs are taken by other cooperative launches: the same plan on one workgroup per window, the same bits
    const bool timed = o->max_solver_time_in_seconds > 0.0 && !o->fixed_iterations;
    const int khz = (coop || timed) ? wall_clock_khz() : 0;      // the cooperative time-out and the solver's time budget count its ticks
    int grid = b->shape.grid;
    b->last.last_wg = coop ? 1 + b->coop.h : 1;
    if (coop) {
        a.coop_h = b->coop.h; a.coop_groups = b->coop.groups; a.coop_exp_chunks = b->coop.exp_chunks; a.coop_exp_stride = b->coop.exp_stride;
        a.coop_ctl = b->coop.d_ctl; a.coop_x = b->coop.d_x; a.coop_exp = b->coop.d_exp; a.coop_rot = b->claim.rot;
        a.coop_timeout = (long long)khz * 2000;      // 2 s
    } else if (b->coop.h > 0) grid = b->shape.slots;
    b->last.sqrt_out_valid = b->mem.d_sqrt_out != nullptr;
    if (const char *sk = getenv("TCV_ABLATE_SKIP")) a.pad2 = (int)(unsigned)strtoul(sk, nullptr, 0);      // -DTCV_ABLATE builds only read it
    if (timed) {
        a.max_ticks = (long long)(o->max_solver_time_in_seconds * 1e3 * (double)khz);
        if (a.max_ticks < 1) a.max_ticks = 1;
    }
    if (int rc = b->flight.enter(st)) return rc;
    if (coop) HIPCHK(hipMemsetAsync(b->coop.d_ctl, 0, sizeof(int) * (size_t)b->coop.groups * COOP_CTL_INTS, st));
    HIPCHK(hipEventRecord(b->last.ev0, st));
    const int rc = tcv_launch_solve(&a, grid, (!b->shape.chain && o->threads_per_window == 512) ? 512 : 256, b->shape.lds_bytes, (void *)st);
    if (rc != 0) return hip_fail((hipError_t)rc, "solve kernel launch");
    HIPCHK(hipEventRecord(b->last.ev1, st));
    b->last.solved = true;
    if (ReloState *r = tcv_relo_of(b)) r->done = false;
    b->last.gauge_in_solve = a.gauge_fix != 0;
    return TCV_OK;
}
extern "C" int tcv_batch_marginalize(tcv_batch *b, void *hip_stream) {
    if (!b) return TCV_ERR_INVALID;
    const hipStream_t st = tcv::resolve_stream(hip_stream);
    if (int rc = b->flight.enter(st)) return rc;
    return tcv_marg_run(b, (void *)st);
}
extern "C" int tcv_batch_synchronize(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (hipError_t e = b->flight.wait_all()) return hip_fail(e, "wait for the batch's streams");
    b->solve_finished();
    tcv_marg_elapsed(b);
    return TCV_OK;
}
// TCV_PROFILE builds only: copies (and clears) the 32 per-phase cycle accumulators of the solve kernel
extern "C" int tcv_batch_profile(tcv_batch *b, double *out32) {
    if (!b || !out32) return TCV_ERR_INVALID;
    std::vector<double> h((size_t)32 * b->shape.slots);
    HIPCHK(hipMemcpy(h.data(), b->mem.d_prof, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < 32; i++) { out32[i] = 0; for (int g = 0; g < b->shape.slots; g++) out32[i] += h[(size_t)g * 32 + i]; }
    HIPCHK(hipMemset(b->mem.d_prof, 0, sizeof(double) * h.size()));
    return TCV_OK;
}
extern "C" int tcv_batch_cooperative(const tcv_batch *b, int *helpers, int *groups, int *chunks, int *last_solve_workgroups) {
    if (!b) return TCV_ERR_INVALID;
    if (last_solve_workgroups) *last_solve_workgroups = b->last.last_wg;
    if (helpers) *helpers = b->coop.h;
    if (groups) *groups = b->coop.h > 0 ? b->coop.groups : 0;
    if (chunks) { int c = 0; for (auto &H : b->in.plans) c = std::max(c, H.n_vis_chunk); *chunks = c; }
    return TCV_OK;
}
// developer diagnostics: the control block of group `group` (COOP_CTL_INTS ints: request / served sequence numbers, abort flag, progress
// marks), copied on a private stream so that it can be read while a launch is still running
extern "C" int tcv_batch_debug_coop(tcv_batch *b, int group, int *out64) {
    if (!b || !out64 || b->coop.h <= 0 || group < 0 || group >= b->coop.groups) { set_error("debug_coop: no cooperative plan / bad group"); return TCV_ERR_INVALID; }
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipError_t e = hipMemcpyAsync(out64, b->coop.d_ctl + (size_t)group * COOP_CTL_INTS, sizeof(int) * COOP_CTL_INTS, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return hip_fail(e, "debug_coop copy");
    return TCV_OK;
}
extern "C" int tcv_batch_layout(const tcv_batch *b) { return b ? (b->shape.chain ? 0 : 1) : TCV_ERR_INVALID; }
extern "C" int tcv_batch_plan_stats(tcv_batch *b, int *num_plans, double *plan_bytes, int *grid, int *lds_bytes) {
    if (!b) return TCV_ERR_INVALID;
    if (num_plans) *num_plans = (int)b->in.plans.size();
    if (plan_bytes) *plan_bytes = b->in.plan_bytes;
    if (grid) *grid = b->shape.grid;
    if (lds_bytes) *lds_bytes = (int)b->shape.lds_bytes;
    return TCV_OK;
}
