// C-ABI of include/tcv.h: what comes back from a device-resident batch -- the states (at once, or split into begin / end around more
// work), summaries, the first step, the priors as handles or downloads, the statistics -- and the single-problem conveniences tcv_solve
// and tcv_marginalize.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tcv_host.h"
#include "tcv_relo.h"      // RELO_REC: the relocalisation record that rides with the states

using namespace tcv;

// the solved states (StateDownload::h_state) into the callers' parameter blocks: camera blocks in plan order, then the inverse depths
static void scatter_states(const tcv_batch *b) {
    for (int w = 0; w < b->in.n; w++) {
        const Packed &pk = b->in.packed[w];
        const tcv_problem &p = *b->in.problems[w];
        const double *x = b->dl.h_state.data() + (size_t)w * b->in.state_stride;
        int off = 0;
        for (int blk : pk.cam_block) { std::memcpy(p.blocks[blk].addr, x + off, sizeof(double) * p.blocks[blk].size); off += p.blocks[blk].size; }
        for (int blk : pk.lm_block) p.blocks[blk].addr[0] = x[off++];
    }
}
extern "C" int tcv_batch_download_states(tcv_batch *b) {
    if (!b || !b->last.solved) return TCV_ERR_INVALID;
    if (tcv_relo_of(b)) return tcv_batch_download_states_brief(b, nullptr, nullptr, nullptr);      // (the relocalisation records ride with the states, and their `valid` needs the terminations)
    if (int rc = b->settle()) return rc;
    b->dl.h_state.resize((size_t)b->in.n * b->in.state_stride);
    if (int rc = tcv::staged_download(b->dl.h_state.data(), b->mem.d_state, sizeof(double) * b->dl.h_state.size(), "download of the states")) return rc;
    scatter_states(b);
    return TCV_OK;
}
// Split form for callers that enqueue more work behind the solve: _begin puts the copy of the states (and of the summary heads) on `hip_stream`
// behind whatever the batch has in flight there and returns; the caller may launch the marginalisation right behind it; _end waits for the
// COPY only (an event), not for the stream, and hands the results out.  The native estimator does: the marginalisation starts the moment the
// states have left, not a host round trip later.
extern "C" int tcv_batch_download_states_begin(tcv_batch *b, void *hip_stream) {
    if (!b || !b->last.solved) return TCV_ERR_INVALID;
    if (b->dl.dl_staging) { set_error("batch_download_states_begin: a download is in flight already"); return TCV_ERR_INVALID; }
    const hipStream_t st = tcv::resolve_stream(hip_stream);
    if (int rc = b->flight.enter(st)) return rc;
    b->dl.h_state.resize((size_t)b->in.n * b->in.state_stride);
    const size_t sbytes = sizeof(double) * b->dl.h_state.size(), hbytes = (size_t)32 * b->in.n;
    ReloState *r = tcv_relo_of(b);
    const bool relo = r && r->done;      // the relocalisation records of tcv_batch_gauge_fix (tcv_relo.hip) in the same round trip
    const size_t rbytes = relo ? sizeof(double) * (size_t)tcv::RELO_REC * r->n : 0;
    static_assert(offsetof(DevSummary, final_cost) == 24 && offsetof(DevSummary, num_iterations) == 0 && offsetof(DevSummary, termination) == 4, "head of DevSummary");
    char *hs = (char *)host_staging_acquire(sbytes + hbytes + rbytes);
    if (!hs) { set_error("hipHostMalloc (download staging) failed"); return TCV_ERR_HIP; }
    hipError_t e_ = hipSuccess;
    if (!b->dl.ev_dl) e_ = hipEventCreateWithFlags(&b->dl.ev_dl, hipEventDisableTiming);
    if (e_ == hipSuccess) e_ = hipMemcpyAsync(hs, b->mem.d_state, sbytes, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess) e_ = hipMemcpy2DAsync(hs + sbytes, 32, b->mem.d_summary, sizeof(DevSummary), 32, (size_t)b->in.n, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess && relo) e_ = hipMemcpyAsync(hs + sbytes + hbytes, r->d, rbytes, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess) e_ = hipEventRecord(b->dl.ev_dl, st);
    if (e_ != hipSuccess) { (void)tcv::stream_wait(st); host_staging_release(hs); return hip_fail(e_, "download of the states"); }
    b->dl.dl_staging = hs;
    if (r) r->in_dl = relo;
    return TCV_OK;
}
extern "C" int tcv_batch_download_states_end(tcv_batch *b, int *num_iterations, int *termination, double *final_cost) {
    if (!b || !b->dl.dl_staging || !b->dl.ev_dl) { set_error("batch_download_states_end: no download in flight"); return TCV_ERR_INVALID; }
    char *hs = (char *)b->dl.dl_staging;
    const size_t sbytes = sizeof(double) * b->dl.h_state.size();
    const hipError_t e_ = hipEventSynchronize(b->dl.ev_dl);
    if (e_ == hipSuccess) {
        std::memcpy(b->dl.h_state.data(), hs, sbytes);
        for (int w = 0; w < b->in.n; w++) {
            const char *q = hs + sbytes + (size_t)32 * w;
            int it, tm; double fc;
            std::memcpy(&it, q, 4); std::memcpy(&tm, q + 4, 4); std::memcpy(&fc, q + 24, 8);
            if (num_iterations) num_iterations[w] = it;
            if (termination) termination[w] = tm;
            if (final_cost) final_cost[w] = fc;
        }
        ReloState *r = tcv_relo_of(b);
        if (r && r->in_dl) {
            r->h_rec.resize((size_t)tcv::RELO_REC * r->n);
            std::memcpy(r->h_rec.data(), hs + sbytes + (size_t)32 * b->in.n, sizeof(double) * r->h_rec.size());
            r->valid.assign(r->n, 0);
            for (int k = 0; k < r->n; k++) {
                int tm;
                std::memcpy(&tm, hs + sbytes + (size_t)32 * r->win[k] + 4, 4);
                r->valid[k] = tm != 5;      // FAILURE: the window's states are not a solution, neither is its record
            }
        }
        if (r) r->have = r->in_dl;
    }
    host_staging_release(hs);
    b->dl.dl_staging = nullptr;
    if (e_ != hipSuccess) return hip_fail(e_, "download of the states");
    b->solve_finished();      // (the solve and the gauge fix lie behind the copy on the stream)
    scatter_states(b);
    return TCV_OK;
}
// States into the callers' blocks AND the three numbers of the summary a per-frame caller reads (the reference reads one:
// summary.iterations.size(), estimator.cpp:1902) in ONE device round trip: the states and the heads of the summary records (32 of their
// 4 136 bytes, a pitched copy) on the calling thread's stream, one wait.
extern "C" int tcv_batch_download_states_brief(tcv_batch *b, int *num_iterations, int *termination, double *final_cost) {
    if (!b || !b->last.solved) return TCV_ERR_INVALID;
    if (int rc = b->settle()) return rc;
    if (int rc = tcv_batch_download_states_begin(b, (void *)tcv::util_stream())) return rc;
    const int rc = tcv_batch_download_states_end(b, num_iterations, termination, final_cost);
    if (rc == TCV_OK) { if (int rcs = tcv_batch_synchronize(b)) return rcs; }      // (nothing of this call stays in flight)
    return rc;
}
static void summary_to_public(const DevSummary &s, tcv_solver_summary *o) {
    std::memset(o, 0, sizeof *o);
    o->num_iterations = s.num_iterations; o->termination = s.termination;
    o->initial_cost = s.initial_cost; o->final_cost = s.final_cost;
    for (int i = 0; i < TCV_MAX_TRACE; i++) {
        o->cost[i] = s.cost[i]; o->cost_candidate[i] = s.cost_candidate[i]; o->model_cost_change[i] = s.model_cost_change[i];
        o->radius[i] = s.radius[i]; o->mu[i] = s.mu[i]; o->rho[i] = s.rho[i]; o->step_norm[i] = s.step_norm[i];
        o->step_ok[i] = s.step_ok[i]; o->dogleg_case[i] = s.dogleg_case[i];
    }
}
extern "C" int tcv_batch_get_summaries(tcv_batch *b, tcv_solver_summary *out, int n) {
    if (!b || !out || n < 0 || n > b->in.n) { set_error("batch_get_summaries: n exceeds the batch size"); return TCV_ERR_INVALID; }
    if (int rc = b->settle()) return rc;
    std::vector<DevSummary> h(n);
    if (int rc = tcv::staged_download(h.data(), b->mem.d_summary, sizeof(DevSummary) * (size_t)n, "download of the summaries")) return rc;
    for (int i = 0; i < n; i++) summary_to_public(h[i], out + i);
    return TCV_OK;
}
// tangent step of iteration 1 in problem order: free camera blocks in the order they were added
// (local size each), then the inverse depths in landmark order.  Returns the length in *len.
extern "C" int tcv_batch_get_first_step(tcv_batch *b, int window, double *out, int cap, int *len) {
    if (!b || window < 0 || window >= b->in.n || !out) return TCV_ERR_INVALID;
    const PlanHdr &H = b->in.plans[b->in.wins[window].plan];
    if (int rc = b->settle()) return rc;
    std::vector<double> d(b->in.delta_stride);
    if (int rc = tcv::staged_download(d.data(), b->mem.d_delta + (size_t)window * b->in.delta_stride, sizeof(double) * b->in.delta_stride, "download of the first step")) return rc;
    const tcv_problem &p = *b->in.problems[window];
    const Packed &pk = b->in.packed[window];
    int k = 0;
    const std::vector<int> &loff = pk.cam_loff;
    for (size_t c = 0; c < pk.cam_block.size(); c++) {
        if (loff[c] < 0) continue;
        const ParamBlock &pb = p.blocks[pk.cam_block[c]];
        const int ls = pb.kind == KIND_POSE ? 6 : pb.size;
        for (int j = 0; j < ls; j++) { if (k >= cap) return TCV_ERR_INVALID; out[k++] = d[loff[c] + j]; }
    }
    for (int l = 0; l < H.nland; l++) { if (k >= cap) return TCV_ERR_INVALID; out[k++] = d[H.nc + l]; }
    if (len) *len = k;
    return TCV_OK;
}
extern "C" int tcv_batch_get_prior(tcv_batch *b, int window, tcv_prior **out) {
    if (!b || !out) return TCV_ERR_INVALID;
    if (int rc = b->settle()) return rc;
    return tcv_marg_get_prior(b, window, out);
}
extern "C" int tcv_batch_get_priors(tcv_batch *b, tcv_prior **out, int n) {
    if (!b || !out || n != b->in.n) { set_error("batch_get_priors: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    if (int rc = b->settle()) return rc;
    const tcv::HostOp host_op;
    const int nth = host_op.threads(std::max(1, std::min(n / 16, 8)));
    std::vector<int> rcs(nth, TCV_OK);
    std::vector<std::string> msgs(nth);
    auto work = [&](int t) {
        // a worker thread starts on device 0: the batch's buffers live on its own device.  The CALLER runs this lambda too (parallel_run):
        // whatever thread it is, its current device is put back
        int prev = -1;
        if (nth > 1 && hipGetDevice(&prev) == hipSuccess && prev != b->shape.dev) (void)hipSetDevice(b->shape.dev); else prev = -1;
        for (int k = t; k < n; k += nth) {
            if (!tcv_marg_has_problem(b, k)) continue;      // not marginalised: out[k] stays NULL
            const int rc = tcv_marg_get_prior(b, k, &out[k]);
            if (rc != TCV_OK) { rcs[t] = rc; msgs[t] = tcv_last_error(); break; }
        }
        if (prev >= 0) (void)hipSetDevice(prev);
    };
    tcv::parallel_run(nth, work);
    for (int t = 0; t < nth; t++)
        if (rcs[t] != TCV_OK) {
            for (int k = 0; k < n; k++) if (out[k]) { tcv_prior_destroy(out[k]); out[k] = nullptr; }
            set_error(msgs[t]);
            return rcs[t];
        }
    return TCV_OK;
}
extern "C" int tcv_batch_get_priors_device_async(tcv_batch *b, tcv_prior **out, int n) {
    if (!b || !out || n != b->in.n) { set_error("batch_get_priors_device_async: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    const int rc = tcv_marg_get_priors_device(b, out, n, true);      // (no wait: the marginalisation may still be running)
    if (rc == TCV_OK && b->flight.pending && !b->flight.streams.empty()) {
        // the batch outlives this call with work in flight: from here on that work is an event, not the streams it runs on -- the calling
        // thread may end (its stream goes with it) before somebody asks for the status or destroys the batch
        (void)tcv_marg_status_prefetch(b, (void *)b->flight.last_stream);
        if (b->flight.track_by_event() != hipSuccess) {
            // no event to track the work by: wait for it here (the streams are still this batch's) -- the handles stay valid, the call merely
            // was not asynchronous; if even that fails the handles are destroyed: "on an error out[] is all NULL" (include/tcv.h)
            const int rcs = tcv_batch_synchronize(b);
            if (rcs != TCV_OK) { for (int k = 0; k < n; k++) if (out[k]) { tcv_prior_destroy(out[k]); out[k] = nullptr; } return rcs; }
            return TCV_OK;
        }
    }
    return rc;
}
extern "C" int tcv_batch_get_priors_device(tcv_batch *b, tcv_prior **out, int n) {
    if (!b || !out || n != b->in.n) { set_error("batch_get_priors_device: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    if (int rc = b->settle()) return rc;
    return tcv_marg_get_priors_device(b, out, n, false);
}
extern "C" int tcv_batch_download_priors(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (int rc = b->settle()) return rc;
    return tcv_marg_download(b, 0);
}
extern "C" int tcv_batch_download_priors_compact(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (int rc = b->settle()) return rc;
    return tcv_marg_download(b, 1);
}
extern "C" int tcv_batch_stats(tcv_batch *b, double *input_bytes, double *solve_ms, double *marg_ms) {
    if (!b) return TCV_ERR_INVALID;
    if (input_bytes) *input_bytes = b->in.input_bytes;
    if (solve_ms) *solve_ms = b->last.solve_ms;
    if (marg_ms) *marg_ms = b->last.marg_ms;
    return TCV_OK;
}

// ceres::Solve(options, &problem, &summary)   estimator.cpp:1900
extern "C" int tcv_solve(const tcv_solver_options *o, tcv_problem *p, tcv_solver_summary *summary) {
    if (!o || !p) return TCV_ERR_INVALID;
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    int rc = tcv_batch_create(&b, arr, nullptr, nullptr, nullptr, 1);
    if (rc != TCV_OK) return rc;
    rc = tcv_batch_solve(b, o, nullptr);
    if (rc == TCV_OK) rc = tcv_batch_synchronize(b);
    tcv_solver_summary s;
    if (rc == TCV_OK) rc = tcv_batch_get_summaries(b, &s, 1);
    if (rc == TCV_OK) {
        if (summary) *summary = s;
        if (!(s.final_cost == s.final_cost) || s.termination == 5) {
            set_error("solver failure (NaN cost or no valid step); parameter blocks left untouched");
            rc = TCV_ERR_NUMERIC;
        } else rc = tcv_batch_download_states(b);
    }
    tcv_batch_destroy(b);
    return rc;
}

// single-window MarginalizationInfo path (marginalization_factor.cpp:89-321): a batch of one
extern "C" int tcv_marginalize(tcv_problem *p, double *const *drop, int num_drop, tcv_prior **out) {
    if (!p || !drop || num_drop <= 0 || !out) return TCV_ERR_INVALID;
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    double *const *dr[1] = {drop};
    int nd[1] = {num_drop};
    // the marginalisation problem doubles as the (unused) solve problem of the batch
    int rc = tcv_batch_create(&b, arr, arr, dr, nd, 1);
    if (rc != TCV_OK) return rc;
    rc = tcv_batch_marginalize(b, nullptr);
    if (rc == TCV_OK) rc = tcv_batch_synchronize(b);
    if (rc == TCV_OK) rc = tcv_batch_get_prior(b, 0, out);
    tcv_batch_destroy(b);
    return rc;
}
