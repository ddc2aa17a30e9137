// Native estimator: the lock-step frame (solveOdometry :1476-1490, prior chaining :2027-2044 / :2083-2113 of estimator.cpp) -- the full
// windows of a list of estimators as ONE device batch: the ticket of tcv_estimators_optimize_begin / _end and its phases, the frame left in
// flight behind it, and the host and kernel time accounts.
// Host code only: every numerical step of the hot path goes through the C-ABI of tcv.h (HIP kernels); there is no CPU solver here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>

#include "tcv_est.h"
#include "tcv_hostpool.h"      // parallel_items, async_run, HostOp: the persistent host worker threads
#include "tcv_runtime.h"       // util_stream, aux_stream, set_error

using namespace tcv_est;

int tcv_marg_layout_n(const tcv_batch *b, int window);      // (tcv_marg_host.cpp: n of the prior a window's attached marginalisation problem makes, known before the kernel runs)

// kernel-time accounting of the lock-step frames (tcv_estimators_kernel_profile): HIP-event durations of the solve and marginalisation
// launches, the windows they held and those windows' ALGORITHMIC bytes x linearisations -- what bench.py --mode replay
// prices against the HBM roofline
static std::mutex g_kmu;
static double g_kern[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // solve ms, solve launches, marginalisation ms, marginalisation launches, windows, bytes x linearisations, linearisations, marginalised windows
static void kern_add(int slot, double v) { std::lock_guard<std::mutex> g(g_kmu); g_kern[slot] += v; }

// A lock-step frame whose marginalisation was left running when tcv_estimators_optimize returned (device-resident state): its batch,
// shared by the estimators of the frame; each asks for the status of its own window at its next frame (or lets go of it when
// it is reset / destroyed), the last one to let go destroys the batch.
struct EstInflight {
    tcv_batch *b = nullptr;
    int n_marg = 0;
    // deferred launch (frames of many windows): the frame that solved the batch returns WITHOUT launching its marginalisation; the first of
    // its estimators to come back for its next frame launches it -- behind that frame's 2D-3D association, whose device round trip would
    // otherwise queue behind the marginalisation kernel on the thread's stream (0.3 - 0.5 ms of a lock-step frame, whatever the number
    // of windows) -- and every estimator takes its own prior handle.  The kernel then runs while the host builds that frame's windows.
    bool launched = false;
    int launch_rc = TCV_OK;
    std::string launch_msg;
    std::vector<tcv_prior *> handles;      // per window of the batch: the new prior, until its estimator takes it
    int launch(void *stream) {      // (any estimator of the batch, any thread: once)
        std::lock_guard<std::mutex> g(mu);
        if (launched) return launch_rc;
        launched = true;
        const int n = tcv_batch_size(b);
        handles.assign(n, nullptr);
        // (test hook: TCV_EST_INJECT_LAUNCH_FAIL=q makes the q-th deferred launch of the process fail -- the library has no natural one to offer)
        static std::atomic<int> launches{0};
        static const int inject = getenv("TCV_EST_INJECT_LAUNCH_FAIL") ? atoi(getenv("TCV_EST_INJECT_LAUNCH_FAIL")) : -1;
        if (inject >= 0 && launches.fetch_add(1) == inject) { tcv::set_error("injected launch failure"); launch_rc = TCV_ERR_HIP; }
        else launch_rc = tcv_batch_marginalize(b, stream);
        if (launch_rc == TCV_OK) launch_rc = tcv_batch_get_priors_device_async(b, handles.data(), n);
        if (launch_rc != TCV_OK) launch_msg = tcv_last_error();
        return launch_rc;
    }
    tcv_prior *take(int k) { std::lock_guard<std::mutex> g(mu); tcv_prior *p = (k >= 0 && k < (int)handles.size()) ? handles[k] : nullptr; if (p) handles[k] = nullptr; return p; }
    std::vector<int> status;
    bool have_status = false;
    std::mutex mu;
    int status_of(int k) {
        std::lock_guard<std::mutex> g(mu);
        if (!have_status) {
            const int n = tcv_batch_size(b);
            status.assign(n, -9);
            if (tcv_batch_marg_status(b, status.data(), n) != TCV_OK) status.assign(n, -9);      // (waits for the batch; -9: the question itself failed)
            have_status = true;
        }
        // (test hook: TCV_EST_INJECT_MARG_FAIL=q reports the q-th status asked for in the process as a sweep-cap failure)
        static std::atomic<int> asked{0};
        static const int inject = getenv("TCV_EST_INJECT_MARG_FAIL") ? atoi(getenv("TCV_EST_INJECT_MARG_FAIL")) : -1;
        if (inject >= 0 && asked.fetch_add(1) == inject) return 1;
        return (k >= 0 && k < (int)status.size()) ? status[k] : -9;
    }
    ~EstInflight() {
        for (tcv_prior *p : handles) if (p) tcv_prior_destroy(p);
        if (!b) return;
        double ms = 0;
        if (tcv_batch_synchronize(b) == TCV_OK && tcv_batch_stats(b, nullptr, nullptr, &ms) == TCV_OK && ms > 0) { kern_add(2, ms); kern_add(3, 1); kern_add(7, n_marg); }
        tcv_batch_destroy(b);      // (waits for work in flight)
    }
};

// host-side time accounting of tcv_estimators_optimize (seconds, cumulative; read and cleared by tcv_estimators_profile):
// 0 pre-integration, 1 association + triangulation + window, 2 problem construction, 3 batch_create (pack + H2D), 4 kernels (launch to
// sync), 5 downloads (states, summaries, priors), 6 apply / prior chaining, 7 calls
// Process-wide state of tcv_estimators_optimize, shared by host threads that drive estimators on the same or on different GPUs: the
// profile accumulators.
namespace {
std::mutex g_mu;
double g_prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
void prof_add(int slot, double v) { std::lock_guard<std::mutex> g(g_mu); g_prof[slot] += v; }
// TCV_DEBUG_EST_CPU=1 (developer): CPU time of the whole process (caller, worker threads, runtime threads) between the laps of the same slots,
// printed by tcv_estimators_profile -- drive the estimators from ONE host thread to read it
double g_prof_cpu[8] = {0, 0, 0, 0, 0, 0, 0, 0};
bool prof_cpu_on() { static const bool on = getenv("TCV_DEBUG_EST_CPU") != nullptr; return on; }
double cpu_now_s() { timespec ts; clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
void prof_cpu_add(int slot, double v) { std::lock_guard<std::mutex> g(g_mu); g_prof_cpu[slot] += v; }
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the time marks of a frame: add(slot) books what has passed since the last mark on a profile slot, wall and (TCV_DEBUG_EST_CPU) process CPU
struct Lap {
    double t = now_s(), c = prof_cpu_on() ? cpu_now_s() : 0.0;
    void add(int slot) {
        const double t1 = now_s(); prof_add(slot, t1 - t); t = t1;
        if (prof_cpu_on()) { const double c1 = cpu_now_s(); prof_cpu_add(slot, c1 - c); c = c1; }
    }
    void mark_cpu() { if (prof_cpu_on()) c = cpu_now_s(); }      // (what the process burns between _begin and _end is not the frame's)
};
// per-estimator host work of a lock-step frame (association bookkeeping, triangulation, window and problem construction) on the packer's
// persistent worker threads: the estimators are independent objects, every task touches its own
void for_each_estimator(int n, const std::function<void(int)> &fn) {
    tcv::HostOp op;
    const int nth = op.threads(n);
    if (nth <= 1) { for (int i = 0; i < n; i++) fn(i); return; }
    tcv::parallel_items(n, nth, [&](int i, int) { fn(i); });
}
}  // namespace
// the same for tasks that can fail: every task's code and, where it failed, the error text of the thread it ran on (the text is per thread)
std::vector<TaskRc> tcv_est::for_each_estimator_rc(int n, const std::function<int(int)> &fn, bool on_caller) {
    std::vector<TaskRc> r(n);
    auto one = [&](int i) { r[i].rc = fn(i); if (r[i].rc != TCV_OK) r[i].msg = tcv_last_error(); };
    if (on_caller) for (int i = 0; i < n; i++) one(i); else for_each_estimator(n, one);
    return r;
}
// the first failure in index order, its text on the calling thread; rcs_out (one int per task), when given, takes every code
int tcv_est::first_failure(const std::vector<TaskRc> &r, int *rcs_out) {
    if (rcs_out) for (size_t i = 0; i < r.size(); i++) rcs_out[i] = r[i].rc;
    for (const TaskRc &t : r) if (t.rc != TCV_OK) { tcv::set_error(t.msg); return t.rc; }
    return TCV_OK;
}
extern "C" int tcv_estimators_kernel_profile(double *out8) {
    if (!out8) return TCV_ERR_INVALID;
    std::lock_guard<std::mutex> g(g_kmu);
    for (int i = 0; i < 8; i++) { out8[i] = g_kern[i]; g_kern[i] = 0; }
    return TCV_OK;
}
extern "C" int tcv_estimators_profile(double *out8) {
    if (!out8) return TCV_ERR_INVALID;
    std::lock_guard<std::mutex> g(g_mu);
    if (prof_cpu_on() && g_prof[7] > 0) {
        static const char *nm[7] = {"preintegrate", "assoc+triangulate+window", "problems", "batch_create", "kernels", "downloads", "apply"};
        for (int i = 0; i < 7; i++) fprintf(stderr, "[est cpu] %-26s wall %8.3f ms  process cpu %8.3f ms per call (%.0f calls)\n", nm[i], 1e3 * g_prof[i] / g_prof[7], 1e3 * g_prof_cpu[i] / g_prof[7], g_prof[7]);
    }
    for (int i = 0; i < 8; i++) { out8[i] = g_prof[i]; g_prof[i] = 0; g_prof_cpu[i] = 0; }
    return TCV_OK;
}

// ---- a lock-step frame in two halves (tcv_estimators_optimize_begin / _end): everything up to the last command on the device, and the wait
// for the states with what follows.  The ticket is the frame's record: what the first half leaves for the second.
//
// One device batch per frame: the windows that marginalise (MARGIN_OLD, or MARGIN_SECOND_NEW with para_Pose[WINDOW_SIZE - 1] in the prior,
// estimator.cpp:2049-2050) carry a marginalisation problem, the others a NULL entry (tcv_batch_create).
// Every kernel of the frame goes on the CALLING THREAD's utility stream -- the stream tcv_batch_create's uploads, the device-to-device
// splices and the downloads of this thread use anyway: host threads that drive their own estimators overlap on the device (a stream pair
// shared by the threads of a device, as until round 4, serialises their kernels: 8 streams on 4 host threads 1 000 against 2 400 windows/s),
// and with one stream per thread no small copy of one thread waits behind another thread's 2 ms solve kernel on a shared hardware queue.
//
// The new prior of a window reaches its estimator in one of two ways (host_priors):
//  - on the device (the default).  last_marginalization_info stays there (estimator.h:176-177: the reference keeps it alive between frames,
//    too): the new priors are handles on the batch's result buffer, the next frame's tcv_batch_create splices them device-to-device.  The
//    host then needs nothing of the marginalisation but its status: the frame is over once the solve and the gauge fix are done and the
//    states are applied; the marginalisation is launched behind them and runs while the caller finishes the frame and starts the next one
//    (tcv_batch_get_priors_device_async).  Its status is read at each estimator's NEXT frame, after that frame's solve: a window solved
//    on a prior whose marginalisation failed is not applied and reports the failure (finish_frame), one frame late.  Faster at every batch
//    size once every host thread launches on its own stream (512-window passes: 171 K against 117 K windows/s; eight replay streams on two
//    host threads: 2 370 - 2 480 against 2 250 - 2 280 windows/s).
//  - TCV_EST_HOST_PRIORS=1: round 3's host round trip (62 KB down, 46 KB up per window), the reference of tests/test_gpu_resident.py --
//    same bits.  The batch is created with its marginalisation problems, the call waits for solve and marginalisation and copies every
//    window's prior to the host.
struct tcv_opt_ticket {
    std::vector<tcv_estimator *> es;
    std::vector<char> dm;             // per window: it marginalises
    bool any_marg = false;
    std::vector<tcv_problem *> P, M;
    std::vector<double *const *> drops;
    std::vector<int> ndrop;
    std::vector<tcv_solver_summary> sum;
    std::vector<tcv_prior *> newp;
    std::vector<tcv_relo_result> relo;   // per window: its relocalisation record (valid = 0: none), read with the states
    std::vector<int> est_rc;          // per estimator: TCV_ERR_NUMERIC when its own window failed
    std::string est_msg;
    tcv_batch *b = nullptr;
    int rc = TCV_OK;                  // the first failure of the batch as a whole: carried to _end, which applies nothing then
    hipStream_t stream = nullptr;
    bool host_priors = false;         // the two hand-over modes above
    bool defer = false;               // the marginalisation of this frame is launched by its estimators' next frame (EstInflight)
    bool dl_begun = false;            // the copy of the states was enqueued behind the solve: _end waits for it
    Lap lap;
    int n() const { return (int)es.size(); }
    ~tcv_opt_ticket() {
        if (b) tcv_batch_destroy(b);
        for (auto *p : P) if (p) tcv_problem_destroy(p);
        for (auto *p : M) if (p) tcv_problem_destroy(p);
        for (auto *p : newp) if (p) tcv_prior_destroy(p);
    }
};

namespace {
int check_ready(const tcv_opt_ticket &T) {
    const int n = T.n();
    for (int i = 0; i < n; i++) if (!T.es[i] || T.es[i]->phase != 1) { tcv::set_error("estimators_optimize: an estimator has no full window waiting (begin_frame must report ready)"); return TCV_ERR_INVALID; }
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (T.es[i] == T.es[j]) { tcv::set_error("estimators_optimize: the same estimator twice"); return TCV_ERR_INVALID; }
    return TCV_OK;
}
// 2D-3D association, first half: per estimator its poses, the detections of its line tracks and its field-of-view sets (independent objects,
// the worker threads share them), then ONE device round trip for all of them
int associate(const tcv_opt_ticket &T, std::vector<AssocJob> &jobs) {
    static const bool dbg = getenv("TCV_DEBUG_EST") != nullptr;      // developer: where this lap goes
    const int n = T.n();
    const double ta0 = now_s();
    bool warm = true;
    for (tcv_estimator *e : T.es) if (e->assoc && !e->fov_ready) warm = false;      // (the first frame's own device call per estimator stays on this thread)
    const int rcp = first_failure(for_each_estimator_rc(n, [&](int i) { return T.es[i]->assoc ? assoc_prepare(T.es[i], jobs[i]) : TCV_OK; }, !warm));
    if (rcp != TCV_OK) return rcp;
    std::vector<tcv_match_lines_args> calls;
    for (int i = 0; i < n; i++) if (T.es[i]->assoc && jobs[i].call) calls.push_back(jobs[i].args);
    const double ta1 = now_s();
    if (!calls.empty()) { const int rc = tcv_match_lines_batch((int)calls.size(), calls.data()); if (rc != TCV_OK) return rc; }
    if (dbg) fprintf(stderr, "[est] n %d: association prepare %.3f ms, device round trip (%d calls) %.3f ms\n", n, 1e3 * (ta1 - ta0), (int)calls.size(), 1e3 * (now_s() - ta1));
    return TCV_OK;
}
// the previous frame's marginalisations (deferred: see EstInflight) go on the device NOW, behind the association's round trip, and every
// estimator takes the prior it will build this frame's window on (getParameterBlocks, marginalization_factor.cpp:301-321)
int launch_pending_marginalizations(const tcv_opt_ticket &T) {
    for (tcv_estimator *e : T.es) {
        if (!e->pend) continue;
        std::shared_ptr<EstInflight> fl = e->pend;
        const int rcl = fl->launch((void *)T.stream);
        if (rcl != TCV_OK) {
            // the launch failed for the whole batch of the previous frame (EstInflight::launch keeps the verdict): every estimator of that batch loses
            // its new prior -- and only those: nothing is sticky, the rest of THIS call's estimators go on, and the affected ones report the failure
            // through finish_frame instead of blocking every later call until a reset (round-5 advisor finding)
            e->pend_failed = rcl; e->pend_msg = fl->launch_msg;
            e->pend.reset(); e->pend_k = -1;
            if (e->prior) { tcv_prior_destroy(e->prior); e->prior = nullptr; }
            e->prior_blocks.clear(); e->stats.prior_n = 0;
            continue;
        }
        tcv_prior *np = fl->take(e->pend_k);
        if (!np) { tcv::set_error("estimators_optimize: the previous frame's marginalisation left no prior for this estimator"); return TCV_ERR_INVALID; }
        const int rct = take_prior(e, np, e->pend_flag);
        if (rct != TCV_OK) { tcv_prior_destroy(np); return rct; }
        e->prev = fl; e->prev_k = e->pend_k;
        e->pend.reset(); e->pend_k = -1;
    }
    return TCV_OK;
}
// one pre-integration call for every stale IMU buffer of every estimator
int preintegrate_stale(const tcv_opt_ticket &T) {
    std::vector<int> first, count;
    std::vector<double> samples, init;
    std::vector<std::pair<tcv_estimator *, int>> who;
    for (tcv_estimator *e : T.es)
        for (int j = 1; j <= W; j++) {
            if (e->pre_valid[j]) continue;
            const ImuBuf &b = e->bufs[j];
            if (!b.valid) { tcv::set_error("estimators_optimize: missing IMU buffer"); return TCV_ERR_INVALID; }
            who.push_back({e, j});
            first.push_back((int)samples.size() / 7); count.push_back((int)b.acc.size());
            for (size_t k = 0; k < b.acc.size(); k++) { samples.push_back(e->cfg.imu_dt); samples.insert(samples.end(), b.acc[k].begin(), b.acc[k].end()); samples.insert(samples.end(), b.gyr[k].begin(), b.gyr[k].end()); }
            init.insert(init.end(), b.acc0.begin(), b.acc0.end()); init.insert(init.end(), b.gyr0.begin(), b.gyr0.end());
            init.insert(init.end(), b.ba.begin(), b.ba.end()); init.insert(init.end(), b.bg.begin(), b.bg.end());
        }
    if (who.empty()) return TCV_OK;
    const tcv_estimator_config &c = T.es[0]->cfg;
    const double noise[4] = {c.acc_n, c.gyr_n, c.acc_w, c.gyr_w};
    if (samples.empty()) samples.push_back(0.0);
    // pre_integrations[] stay on the device (the reference keeps them alive between frames, too): a handle per buffer, sum_dt on the
    // host; nobody waits for the kernel (tcv_preintegrate_device).  TCV_EST_HOST_PREINT=1: round 3's round trip (3.7 KB down per buffer,
    // 2.3 KB up per factor and window), the reference of tests/test_gpu_resident.py -- same bits
    if (getenv("TCV_EST_HOST_PREINT")) {
        std::vector<tcv_imu_preintegration> out(who.size());
        const int rc = tcv_preintegrate((int)who.size(), first.data(), count.data(), samples.data(), (int)samples.size() / 7, init.data(), noise, out.data());
        if (rc != TCV_OK) return rc;
        for (size_t k = 0; k < who.size(); k++) { tcv_estimator *e = who[k].first; e->pre[who[k].second] = out[k]; e->preh[who[k].second].reset(); e->pre_valid[who[k].second] = true; }
        return TCV_OK;
    }
    std::vector<tcv_preint *> hd(who.size(), nullptr);
    const int rc = tcv_preintegrate_device((int)who.size(), first.data(), count.data(), samples.data(), (int)samples.size() / 7, init.data(), noise, hd.data());
    if (rc != TCV_OK) return rc;
    for (size_t k = 0; k < who.size(); k++) {
        tcv_estimator *e = who[k].first;
        const int j = who[k].second;
        e->preh[j] = std::shared_ptr<tcv_preint>(hd[k], tcv_preint_destroy);
        std::memset(&e->pre[j], 0, sizeof e->pre[j]);
        e->pre[j].sum_dt = tcv_preint_sum_dt(hd[k]);
        e->pre_valid[j] = true;
    }
    return TCV_OK;
}
// association, second half, and solveOdometry up to the solver call: triangulation, vector2double + graph
int build_windows(const tcv_opt_ticket &T, std::vector<AssocJob> &jobs) {
    for_each_estimator(T.n(), [&](int i) {
        tcv_estimator *e = T.es[i];
        if (e->assoc) assoc_finish(e, jobs[i]);
        triangulate(e);
        build_window(e);
    });
    for (tcv_estimator *e : T.es) if (e->tap.on) { const int rc = tap_window(e); if (rc != TCV_OK) return rc; }
    return TCV_OK;
}
// the marginalisation problem of window k and the blocks it drops: both hand-over modes build it here, on a worker thread
int build_marg_problem(tcv_opt_ticket &T, int k) {
    tcv_estimator *e = T.es[k];
    tcv_window_desc d;
    build_marg(e, e->marg_flag);
    fill_desc(e, d, true);
    const int rc = tcv_problem_from_window(&d, &T.M[k]);
    T.drops[k] = e->m_drop.data(); T.ndrop[k] = (int)e->m_drop.size();
    return rc;
}
// relo_Pose and its factors behind the window's own (estimator.cpp:1854-1886), then what double2vector's tail needs (:1606-1624)
int add_relocalization(tcv_estimator *e, tcv_problem *p, double sqrt_info, double loss_a) {
    int rc = tcv_problem_add_parameter_block(p, e->relo_pose, 7, TCV_PARAM_POSE);
    for (size_t k = 0; k < e->r_pi.size() && rc == TCV_OK; k++)
        rc = tcv_problem_add_projection_factor(p, e->r_pts.data() + 6 * k, e->r_pts.data() + 6 * k + 3, sqrt_info, loss_a, e->para_pose + 7 * e->r_pi[k], e->relo_pose,
                                               e->para_ex, e->para_feature.data() + e->r_pl[k]);
    if (rc == TCV_OK) rc = tcv_problem_set_relocalization(p, e->relo_pose, e->w_relo_local, e->w_relo_prev, e->w_relo_prev + 3);
    return rc;
}
// every window's problem.  Host priors: a marginalising window's second problem in the same task; priors on the device: the batch is created
// without them, they are built and attached while the solve runs (attach_marginalization)
void build_problems(tcv_opt_ticket &T) {
    T.rc = first_failure(for_each_estimator_rc(T.n(), [&](int k) {
        tcv_estimator *e = T.es[k];
        tcv_window_desc d;
        fill_desc(e, d, false);
        int rc = tcv_problem_from_window(&d, &T.P[k]);
        if (rc == TCV_OK && e->w_relo) rc = add_relocalization(e, T.P[k], d.proj_sqrt_info, d.proj_loss_a);
        return rc == TCV_OK && T.dm[k] && T.host_priors ? build_marg_problem(T, k) : rc;
    }));
}
void create_batch(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK) return;
    const bool with_marg = T.any_marg && T.host_priors;
    T.rc = tcv_batch_create(&T.b, T.P.data(), with_marg ? T.M.data() : nullptr, with_marg ? T.drops.data() : nullptr, with_marg ? T.ndrop.data() : nullptr, T.n());
}
void enqueue_solve(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK) return;
    const tcv_estimator_config &c = T.es[0]->cfg;
    tcv_solver_options o;
    tcv_solver_options_default(&o);
    o.max_num_iterations = c.num_iterations; o.fixed_iterations = c.fixed_iterations;
    if (c.solver_time > 0.0 && !o.fixed_iterations) {      // estimator.cpp:1894-1897 (one budget per batch: include/tcv_estimator.h)
        bool any_old = false;
        for (const tcv_estimator *e : T.es) any_old = any_old || e->marg_flag == MARGIN_OLD;
        o.max_solver_time_in_seconds = c.solver_time * (any_old ? 4.0 / 5.0 : 1.0);
    }
    void *st = (void *)T.stream;
    // double2vector() in the solve kernel's epilogue (the tcv_batch_gauge_fix below is then a no-op): one launch and its gap less per frame;
    // bit for bit the stand-alone kernel's result (tests/test_gpu_gauge.py)
    T.rc = tcv_batch_set_fused_gauge_fix(T.b, 1);
    if (T.rc == TCV_OK) T.rc = tcv_batch_solve(T.b, &o, st);
    if (T.rc == TCV_OK) T.rc = tcv_batch_gauge_fix(T.b, st);
    if (T.host_priors) { if (T.rc == TCV_OK && T.any_marg) T.rc = tcv_batch_marginalize(T.b, st); return; }
    // the copy of the states (and of the summary heads) goes on the stream right behind the gauge fix -- BEFORE the upload of the marginalisation
    // problems attached next, which used to sit between them (a lock-step frame's GPU timeline: 10 us of upload, a fill and their launch gaps,
    // ~35 us before the states left; tools/gpu_calls.md#r05_gpu_z43)
    if (T.rc == TCV_OK) { T.rc = tcv_batch_download_states_begin(T.b, st); T.dl_begun = T.rc == TCV_OK; }
}
// the solve is on the device: the marginalisation problems of the frame, their packing and upload meanwhile
void attach_marginalization(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK || !T.any_marg) return;
    T.rc = first_failure(for_each_estimator_rc(T.n(), [&](int k) { return T.dm[k] ? build_marg_problem(T, k) : TCV_OK; }));
    if (T.rc == TCV_OK) T.rc = tcv_batch_attach_marginalization(T.b, T.M.data(), T.drops.data(), T.ndrop.data());
}
// A frame of a few windows enqueues its marginalisation NOW, while the solve runs, with its no-wait prior handles: the kernel starts the moment
// the states have left instead of a host round trip (wake-up, unpacking, launch) later, which the next frame's association would wait out.
// It runs on the thread's SECOND stream (ordered behind the copy of the states by an event): the next frame's association round trip on
// the main stream then does not queue behind the kernel (0.45 -> 0.2 ms of a 2.4 ms frame: 8 streams on one host thread 3 200 -> 3 700
// windows/s; on two host threads only if the runtime has a hardware queue per stream, GPU_MAX_HW_QUEUES >= 8: 3 400 -> 3 750; otherwise
// no change).
void enqueue_eager_marginalization(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK || !T.any_marg) return;
    T.rc = tcv_batch_marginalize(T.b, (void *)tcv::aux_stream());
    if (T.rc == TCV_OK) T.rc = tcv_batch_get_priors_device_async(T.b, T.newp.data(), T.n());
}

// Errors up to the tap (bad arguments, association, the pending frame's prior, pre-integration) return from here and leave no ticket; from
// problem construction on they are carried in T.rc to optimize_end, which consumes the ticket.
int optimize_begin(tcv_opt_ticket &T) {
    const int n = T.n();
    T.stream = tcv::util_stream();
    prof_add(7, 1);
    if (const int rc = check_ready(T)) return rc;
    // The association's device round trip comes first and the pre-integration of the new IMU buffers is issued behind it (nobody on the host
    // waits for that kernel: its results are spliced into the batch on the device), so the kernel runs while the host builds the windows and problems.
    std::vector<AssocJob> jobs(n);
    if (const int rc = associate(T, jobs)) return rc;
    T.lap.add(1);
    if (const int rc = launch_pending_marginalizations(T)) return rc;
    if (const int rc = preintegrate_stale(T)) return rc;
    T.lap.add(0);
    if (const int rc = build_windows(T, jobs)) return rc;
    T.lap.add(1);

    T.dm.resize(n);
    for (int i = 0; i < n; i++) {
        const tcv_estimator *e = T.es[i];
        bool has = false;
        for (auto &b : e->prior_blocks) if (b.first == 0 && b.second == W - 1) has = true;
        T.dm[i] = e->marg_flag == MARGIN_OLD || (e->prior && has);
        T.any_marg = T.any_marg || T.dm[i];
    }
    T.P.assign(n, nullptr); T.M.assign(n, nullptr); T.drops.assign(n, nullptr); T.ndrop.assign(n, 0); T.newp.assign(n, nullptr);
    T.host_priors = getenv("TCV_EST_HOST_PRIORS") != nullptr;
    // Deferred marginalisation (EstInflight::launch) for frames of many windows, whose host side is long enough to hide the kernel behind the NEXT
    // frame's window construction: 128 streams on two host threads 17.4 K against 15.7 K windows/s.  A frame of a few windows enqueues it here,
    // right behind the copy of its states -- deferred, its 0.45 ms would end up in front of the next frame's upload (8 streams: 3 050 against
    // 3 250 windows/s).  TCV_EST_MARG_DEFER=n: defer from n windows per call on (0: never, 1: always).
    const char *e_defer = getenv("TCV_EST_MARG_DEFER");      // (read per call: the tests switch it)
    const int defer_from = e_defer ? atoi(e_defer) : 12;
    T.defer = !T.host_priors && defer_from > 0 && n >= defer_from;

    build_problems(T);
    T.lap.add(2);
    create_batch(T);
    T.lap.add(3);
    enqueue_solve(T);
    if (!T.host_priors) {
        attach_marginalization(T);
        if (!T.defer) enqueue_eager_marginalization(T);
    }
    return TCV_OK;
}

// the states and the three summary numbers of every window, through tcv_batch_download_states_end or _brief
int download_states(tcv_opt_ticket &T, int (*download)(tcv_batch *, int *, int *, double *)) {
    const int n = T.n();
    std::vector<int> its(n, 0), tms(n, 0);
    std::vector<double> fcs(n, 0.0);
    const int rc = download(T.b, its.data(), tms.data(), fcs.data());
    for (int k = 0; k < n; k++) { T.sum[k].num_iterations = its[k]; T.sum[k].termination = tms[k]; T.sum[k].final_cost = fcs[k]; }
    return rc;
}
void wait_for_states(tcv_opt_ticket &T) {
    T.sum.assign(T.n(), tcv_solver_summary());
    if (T.dl_begun) {      // waits for the copy (an event behind the solve and the gauge fix), not for the marginalisation behind it
        const int rcd = download_states(T, tcv_batch_download_states_end);
        if (T.rc == TCV_OK) T.rc = rcd;
    } else if (T.rc == TCV_OK) T.rc = tcv_batch_synchronize(T.b);      // (host priors: solve and marginalisation)
    double ms = 0;
    if (T.rc == TCV_OK && tcv_batch_stats(T.b, nullptr, &ms, nullptr) == TCV_OK && ms > 0) { kern_add(0, ms); kern_add(1, 1); }
}
// host priors: states + the three summary numbers in one device round trip, then the priors of the whole batch as one blob
void download_to_host(tcv_opt_ticket &T) {
    if (T.rc == TCV_OK) T.rc = download_states(T, tcv_batch_download_states_brief);
    if (T.rc == TCV_OK && T.any_marg) T.rc = tcv_batch_download_priors_compact(T.b);
}
// the relocalisation records came with the states (tcv_batch_download_states_end / _brief): taken before the batch is handed on or destroyed
void collect_relocalizations(tcv_opt_ticket &T) {
    bool any = false;
    for (const tcv_estimator *e : T.es) any = any || e->w_relo;
    if (!any) return;
    T.relo.assign(T.n(), tcv_relo_result());
    for (int k = 0; k < T.n() && T.rc == TCV_OK; k++) {
        std::memset(&T.relo[k], 0, sizeof T.relo[k]);
        if (T.es[k]->w_relo) T.rc = tcv_batch_get_relocalization(T.b, k, &T.relo[k]);
    }
}
// what became of each window: est_rc / est_msg.  A failed window fails alone -- the other estimators of the lock-step batch are applied,
// this one reports the failure from tcv_estimator_finish_frame
void judge_windows(tcv_opt_ticket &T) {
    const int n = T.n();
    T.est_rc.assign(n, TCV_OK);
    if (T.rc != TCV_OK) return;
    double bytes = 0, lin = 0;      // algorithmic bytes of the frame's windows x linearisations (the initial one + one per iteration)
    for (int k = 0; k < n; k++) {
        const tcv_estimator *e = T.es[k];
        const double L = (double)e->sel.size(), pn = e->prior ? (double)e->stats.prior_n : 0.0, nl = (double)std::max(1, T.sum[k].num_iterations);      // (ceres numbering: iteration 0 is the initial linearisation)
        const double per = 8.0 * ((77 + 99 + 7 + L) + 287.0 * e->w.imu.size() + 6.0 * e->w.pi.size() + 9.0 * e->w.lf.size() + 21 + (pn > 0 ? pn * pn + pn + 86 : 0))
                           + 4.0 * (4.0 * e->w.imu.size() + 4.0 * e->w.pi.size() + e->w.lf.size()) + 8.0 * ((171 + L) + 1);
        bytes += per * nl; lin += nl;
    }
    kern_add(4, n); kern_add(5, bytes); kern_add(6, lin);
    for (int k = 0; k < n; k++) {
        // ceres::Solve's FAILURE (no valid step / a cooperative group that timed out): the window's states are not applied
        if (T.sum[k].termination == 5 || !(T.sum[k].final_cost == T.sum[k].final_cost)) { T.est_rc[k] = TCV_ERR_NUMERIC; T.est_msg = "solver failure (no valid step, NaN cost or workgroup time-out)"; }
        tcv_estimator *e = T.es[k];
        if (e->pend_failed != TCV_OK) {
            T.est_rc[k] = e->pend_failed; T.est_msg = "the previous frame's marginalisation could not be launched (" + e->pend_msg + "): this window was solved without its prior";
            e->pend_failed = TCV_OK; e->pend_msg.clear();
        }
        // the marginalisation that made this window's prior was still running when the previous frame returned: its verdict now (it
        // finished before this frame's solve started)
        if (e->prev) {
            const int stp = e->prev->status_of(e->prev_k);
            if (stp != 0 && stp != 2) { T.est_rc[k] = TCV_ERR_NUMERIC; T.est_msg = "the previous frame's marginalisation failed (eigen-solver sweep cap or NaN): this window was solved on an invalid prior"; }
            e->prev.reset(); e->prev_k = -1;      // (the last estimator of that frame to let go destroys its batch)
        }
        if (T.est_rc[k] != TCV_OK && T.newp[k]) { tcv_prior_destroy(T.newp[k]); T.newp[k] = nullptr; }
    }
}
// host priors: every window's new prior out of the downloaded blob, on the workers.  A window whose marginalisation did not converge
// (TCV_ERR_NUMERIC) fails alone; any other error fails the call
void take_host_priors(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK || !T.any_marg) return;
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    const std::vector<TaskRc> r = for_each_estimator_rc(T.n(), [&](int k) {
        if (T.est_rc[k] != TCV_OK || !T.dm[k]) return (int)TCV_OK;
        (void)hipSetDevice(cur_dev);      // (a worker thread's current device is its own: the copy of a window must see the batch's)
        return tcv_batch_get_prior(T.b, k, &T.newp[k]);
    });
    for (int k = 0; k < T.n(); k++) {
        if (r[k].rc == TCV_OK) continue;
        T.est_rc[k] = r[k].rc;
        if (r[k].rc != TCV_ERR_NUMERIC) { T.rc = r[k].rc; tcv::set_error(r[k].msg); break; }
        T.est_msg = r[k].msg;
    }
}
// priors on the device: the batch lives on until its marginalisation has been asked about, shared by the estimators that marginalised
// (the batch alone: its problems were read for the last time by tcv_batch_download_states / tcv_batch_attach_marginalization and go now,
// like the old prior they point to)
void hand_over_batch(tcv_opt_ticket &T) {
    if (T.rc != TCV_OK || !T.any_marg) return;
    const int n = T.n();
    auto fl = std::make_shared<EstInflight>();
    fl->b = T.b;
    T.b = nullptr;
    for (int k = 0; k < n; k++) fl->n_marg += T.dm[k] ? 1 : 0;
    for (int k = 0; k < n; k++) {
        if (!T.dm[k] || T.est_rc[k] != TCV_OK) continue;
        tcv_estimator *e = T.es[k];
        if (T.defer) { e->pend = fl; e->pend_k = k; e->pend_flag = e->marg_flag; const int pn = tcv_marg_layout_n(fl->b, k); if (pn >= 0) e->stats.prior_n = pn; }      // (the new prior's n is part of the attached problem's layout)
        else { e->prev = fl; e->prev_k = k; }
    }
}
// the frame's problems have been read for the last time: destroyed on a worker thread, behind the caller's back
void retire_problems(tcv_opt_ticket &T) {
    auto dead = std::make_shared<std::vector<tcv_problem *>>();
    dead->reserve(2 * T.P.size());
    for (size_t k = 0; k < T.P.size(); k++) { if (T.P[k]) dead->push_back(T.P[k]); if (T.M[k]) dead->push_back(T.M[k]); T.P[k] = T.M[k] = nullptr; }
    tcv::async_run([dead] { for (tcv_problem *q : *dead) tcv_problem_destroy(q); });
}
// double2vector's host half, the statistics and the prior chaining of every window that did not fail
int apply_windows(tcv_opt_ticket &T) {
    for (int k = 0; k < T.n(); k++) {
        tcv_estimator *e = T.es[k];
        e->opt_failed = TCV_OK;
        if (T.est_rc[k] != TCV_OK) {      // this estimator's window failed numerically: nothing is applied, finish_frame reports it
            e->opt_failed = T.est_rc[k]; e->opt_msg = T.est_msg; e->phase = 2;
            continue;
        }
        apply_states(e);
        if (e->w_relo && T.relo[k].valid) {      // the tail of double2vector (:1606-1620); the drift pair stays until the next relocalisation
            const tcv_relo_result &r = T.relo[k];
            tcv_estimator_relo &o = e->relo_out;
            o.valid = 1; o.frame_index = e->w_relo_frame_index; o.frame_serial = e->w_relo_serial;
            std::memcpy(o.drift_correct_r, r.drift_correct_r, sizeof o.drift_correct_r); std::memcpy(o.drift_correct_t, r.drift_correct_t, sizeof o.drift_correct_t);
            std::memcpy(o.relo_relative_t, r.relo_relative_t, sizeof o.relo_relative_t); std::memcpy(o.relo_relative_q, r.relo_relative_q, sizeof o.relo_relative_q);
            o.relo_relative_yaw = r.relo_relative_yaw;
            std::memcpy(o.relo_r, r.relo_r, sizeof o.relo_r); std::memcpy(o.relo_t, r.relo_t, sizeof o.relo_t);
        }
        if (e->tap.on && e->tap.have && e->w_relo) { std::memcpy(e->tap.relo_out, e->relo_pose, sizeof e->tap.relo_out); e->tap.relo_result = T.relo[k]; }
        if (e->tap.on && e->tap.have) {
            WindowTap &tap = e->tap;
            tap.pose_out.assign(e->para_pose, e->para_pose + (W + 1) * 7); tap.sb_out.assign(e->para_sb, e->para_sb + (W + 1) * 9);
            tap.ex_out.assign(e->para_ex, e->para_ex + 7); tap.feat_out = e->para_feature;
            tap.td_out = e->estimate_td ? e->para_td[0] : 0.0;
            tap.iterations = T.sum[k].num_iterations; tap.final_cost = T.sum[k].final_cost; tap.applied = 1;
        }
        e->stats.marg_flag = e->marg_flag; e->stats.n_landmarks = (int)e->sel.size(); e->stats.n_proj = (int)e->w.pi.size(); e->stats.n_line = (int)e->w.lf.size();
        e->stats.n_line_obs = e->n_line_obs_total; e->stats.iterations = T.sum[k].num_iterations; e->stats.termination = T.sum[k].termination; e->stats.final_cost = T.sum[k].final_cost;
        if (!T.dm[k]) e->stats.prior_n = e->prior ? e->stats.prior_n : 0;
        else if (!T.defer) {      // (deferred: the new prior is taken at the start of the next frame; stats.prior_n was set with the hand-over)
            const int rc = take_prior(e, T.newp[k], e->marg_flag);
            if (rc != TCV_OK) return rc;      // (take_prior keeps the old prior on failure: the ticket releases the new one and the ones not handed over yet)
            T.newp[k] = nullptr;
        }
        e->phase = 2;
    }
    return TCV_OK;
}

int optimize_end(tcv_opt_ticket &T) {
    static const bool dbg = getenv("TCV_DEBUG_EST") != nullptr;      // developer: where the "downloads" lap goes
    T.lap.mark_cpu();
    wait_for_states(T);
    T.lap.add(4);
    const double td0 = now_s();
    if (T.host_priors) download_to_host(T);
    collect_relocalizations(T);
    const double td1 = now_s();
    judge_windows(T);
    if (T.host_priors) take_host_priors(T); else hand_over_batch(T);
    const double td2 = now_s();
    if (T.b) { tcv_batch_destroy(T.b); T.b = nullptr; }
    const double td3 = now_s();
    retire_problems(T);
    if (dbg) fprintf(stderr, "[est] n %d: states %.3f ms, priors %.3f ms, batch destroy %.3f ms, problems destroy %.3f ms\n", T.n(),
                     1e3 * (td1 - td0), 1e3 * (td2 - td1), 1e3 * (td3 - td2), 1e3 * (now_s() - td3));
    T.lap.add(5);
    if (T.rc != TCV_OK) return T.rc;      // (nothing is applied; the ticket releases the priors it still holds)
    T.rc = apply_windows(T);
    T.lap.add(6);
    return T.rc;
}
}  // namespace

// The frame in two calls, for callers that overlap the host side of one group of estimators with the device side of another (bench.py --mode
// replay: every host thread alternates between two halves of its streams): _begin returns when the frame's last command is on the device,
// _end waits for the states and applies them.  tcv_estimators_optimize = _begin + _end.  Between the two calls the estimators of the ticket
// must not be touched; the ticket is consumed by _end (also on failure).
extern "C" int tcv_estimators_optimize_begin(tcv_estimator *const *es, int n, tcv_opt_ticket **out) {
    if (!es || n <= 0 || !out) return TCV_ERR_INVALID;
    tcv_opt_ticket *T = new tcv_opt_ticket();
    T->es.assign(es, es + n);
    const int rc = optimize_begin(*T);
    if (rc != TCV_OK) { delete T; T = nullptr; }
    *out = T;
    return rc;
}
extern "C" int tcv_estimators_optimize_end(tcv_opt_ticket *T) {
    if (!T) return TCV_ERR_INVALID;
    const int rc = optimize_end(*T);
    delete T;
    return rc;
}
extern "C" int tcv_estimators_optimize(tcv_estimator *const *es, int n) {
    tcv_opt_ticket *t = nullptr;
    const int rc = tcv_estimators_optimize_begin(es, n, &t);
    if (rc != TCV_OK) return rc;
    return tcv_estimators_optimize_end(t);
}
