// The device-resident batch behind the C-ABI of include/tcv.h, in parts: what went in, the device memory, the launch shape, the
// cooperative plan and claim, the streams in flight, what the last solve did, the state download -- and the four side states (marginalisation,
// evaluation, covariance, relocalisation), each owned through the same base.  Every part states its invariant and has its own release();
// the ORDER of the releases is batch_free's alone (tcv_batch_create.cpp).
#pragma once
#include "tcv_host.h"
#include "tcv_coop_policy.h"

namespace tcv {

// what the caller handed in and its packed form; fixed once tcv_batch_create returns
struct BatchInputs {
    int n = 0;
    std::vector<tcv_problem *> problems;
    std::vector<Packed> packed;             // host copies of per-window maps (ints/doubles released after upload)
    std::vector<PlanHdr> plans;             // the DISTINCT plans; WinHdr::plan indexes them
    std::vector<long long> plan_base;
    std::vector<WinHdr> wins;
    int state_stride = 0, delta_stride = 0;
    double input_bytes = 0, plan_bytes = 0;
};

// The device buffers.  Four pointers own an allocation of their own kind (d_input, d_zero: one blob with views into it); release() is the
// only code that knows which are owners and which are views.  All come from the process-wide pool (tcv_runtime.h dev_malloc).
struct BatchMemory {
    void *d_input = nullptr;                // one allocation: [data pool | window headers | plan headers | plan offsets | plan ints | splice jobs | device-only tail: the regions of device-resident priors]
    double *d_dpool = nullptr;              // views into d_input
    WinHdr *d_win = nullptr;
    PlanHdr *d_plans = nullptr;
    long long *d_plan_base = nullptr;
    int *d_ipool = nullptr;
    void *d_zero = nullptr;                 // one allocation, zeroed by one memset: [d_delta | d_scratch | d_summary | d_prof]
    double *d_delta = nullptr, *d_scratch = nullptr;      // views into d_zero
    DevSummary *d_summary = nullptr;
    double *d_prof = nullptr;
    double *d_state = nullptr;
    double *d_imublk = nullptr, *d_spill = nullptr;       // chain mode: per-workgroup IMU J'J blocks and factored fronts
    double *d_sqrt_out = nullptr;           // per window 225 doubles: the solve's sqrt_info of the IMU factor the marginalisation needs
    void release();
};

// how the solve is launched: a function of the packed batch and of the device, fixed at creation
struct LaunchShape {
    int dev = 0, n_cu = 0;                  // the device the batch lives on and its CUs
    bool chain = false;                     // all plans use the chain layout (2 workgroups per CU)
    bool chain_td = false;                  // a window has ProjectionTdFactors or wider camera vectors (PlanHdr::camw): the kernel instance that takes them
    int chain_lds = 0;                      // LDS doubles per chain-layout workgroup of this batch
    int grid = 0, slots = 0;                // workgroups; scratch slots (= grid without the cooperative mode, its groups with it)
    size_t lds_bytes = 0;
    int spill_stride = 0;
    int hcl_cap = 0;                        // doubles of the landmark/camera coupling store per workgroup (largest window of the batch)
};

// cooperative mode (tcv_packed.h COOP_*): helpers per window group (0: off, and nothing else here is used), groups, the export layout
struct CoopPlan {
    int h = 0, groups = 0;
    int exp_chunks = 0, exp_stride = 0;
    int *d_ctl = nullptr;
    double *d_x = nullptr, *d_exp = nullptr;
    void release();
};

// The streams with work of this batch in flight.  pending: asynchronous work was issued since the last wait.  While it is, that work is
// tracked EITHER by `streams` (every stream it runs on; null: the device) OR, once wait_inflight is set, by ev_inflight alone -- the
// batch then outlives a call whose stream may go with its host thread.
struct BatchFlight {
    hipStream_t last_stream = nullptr;      // stream of the last asynchronous call
    std::vector<hipStream_t> streams;
    bool pending = false;
    hipEvent_t ev_order = nullptr;          // orders a call on a new stream behind the pending work of the previous one (enter)
    hipEvent_t ev_inflight = nullptr;
    bool wait_inflight = false;
    // every asynchronous entry point of a batch passes through here: a call on another stream than the previous one waits (on the device)
    // for the batch's pending work there -- the gauge fix and the marginalisation read what the solve wrote -- and the stream joins the set
    int enter(hipStream_t st);
    // waits for the event or for every stream (the whole device when one of them is the default stream), not for the device: batches driven
    // from different host threads on different streams overlap (bench.py --mode stream).  Nothing is pending afterwards.
    hipError_t wait_all();
    // from here on the work in flight is ev_inflight, recorded on last_stream, not the streams (tcv_batch_get_priors_device_async)
    hipError_t track_by_event();
    void release();                         // the events
};

// what the last tcv_batch_solve did; ev0 / ev1 bracket its kernel
struct LastSolve {
    bool solved = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float solve_ms = 0, marg_ms = 0;        // read from the events once the work has finished (tcv_batch::solve_finished, tcv_marg_elapsed)
    int last_wg = 0;                        // workgroups per window (1: single-workgroup kernel)
    bool sqrt_out_valid = false;            // it wrote BatchMemory::d_sqrt_out (device-computed sqrt_info)
    bool fuse_gauge = false, gauge_in_solve = false;      // tcv_batch_set_fused_gauge_fix: the fix in the solve kernel's epilogue; whether the LAST solve applied it
    void release();
};

// tcv_batch_download_states_begin .. _end: dl_staging != nullptr exactly while a download is in flight, and ev_dl lies behind its copies
struct StateDownload {
    std::vector<double> h_state;
    hipEvent_t ev_dl = nullptr;
    void *dl_staging = nullptr;             // the pinned buffer
    void release();                         // waits for the copy in flight first
};

// A side state of a batch: made by its owner file at first use, destroyed with the batch (behind every wait and the batch's own buffers).
// Each owner has one typed accessor (marg_of, eval_of, cov_of, tcv_relo_of); nothing else casts.
struct SideState { virtual ~SideState() = default; };

// relocalisation (tcv_relo.hip): the windows whose problem carries tcv_problem_set_relocalization.  A batch without one has no ReloState.
struct ReloState : SideState {
    int n = 0;
    std::vector<int> win;                   // window of every table entry
    double *d = nullptr;                    // one allocation: [records x n | prev_relo_t / _r x n | table], tcv_relo.h
    std::vector<double> h_up;               // the upload's host image (alive as long as the batch: the copy is asynchronous)
    bool done = false;                      // the records belong to the last solve (tcv_batch_gauge_fix ran behind it)
    bool in_dl = false;                     // the download in flight carries them
    bool have = false;                      // h_rec / valid hold them
    std::vector<double> h_rec;              // host copy of the records, downloaded with the states
    std::vector<char> valid;                // per entry: the window's solve did not end in FAILURE
    ~ReloState() override;
};
}  // namespace tcv

struct tcv_batch {
    tcv::BatchInputs in;
    tcv::BatchMemory mem;
    tcv::LaunchShape shape;
    tcv::CoopPlan coop;
    tcv::CoopClaim claim;                   // CUs the cooperative launch in flight holds (tcv_coop_policy.h); total == 0: none
    tcv::BatchFlight flight;
    tcv::LastSolve last;
    tcv::StateDownload dl;
    std::unique_ptr<tcv::SideState> marg, eval, cov, relo;      // tcv_marg_host.cpp MargState, tcv_eval_host.cpp EvalState, tcv_cov_host.cpp CovState, ReloState

    // Nothing of this batch is in flight: a copy on the calling thread's stream is not ordered behind the batch's own streams (a
    // marginalisation or a solve launched on another one), so every getter that copies waits for them first.  TCV_OK or an error.
    int settle() { return flight.pending ? tcv_batch_synchronize(this) : (int)TCV_OK; }
    // The last solve has finished (somebody waited for the streams, or for a copy that lies behind it): the CUs its cooperative launch
    // held go back, and its duration is read.
    void solve_finished() {
        tcv::coop_release(shape.dev, &claim);
        if (last.solved) (void)hipEventElapsedTime(&last.solve_ms, last.ev0, last.ev1);
    }
};
inline tcv::ReloState *tcv_relo_of(const tcv_batch *b) { return static_cast<tcv::ReloState *>(b->relo.get()); }
int tcv_relo_attach(tcv_batch *b, hipStream_t upload_stream);      // tcv_batch_create: table + prev_relo_* up, record buffer (no-op without relocalisation problems)
int tcv_relo_launch(tcv_batch *b, hipStream_t st);                 // tcv_batch_gauge_fix: relo_fix_batch_kernel in front of the gauge kernel

