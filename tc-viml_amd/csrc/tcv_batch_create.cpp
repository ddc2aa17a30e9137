// C-ABI of include/tcv.h: the device-resident batch, made and unmade -- tcv_batch_create phase by phase (pack_plans .. alloc_work_buffers),
// the marginalisation problems attached later, the per-plan side tables, and batch_free with the one release order of the batch's parts
// (tcv_batch.h).  Host code only; there is no CPU fallback: without a HIP device every compute entry point returns TCV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "tcv_host.h"

using namespace tcv;

extern "C" int tcv_solve_scratch_doubles(void);
static_assert((int)COOP_POLICY_MAX_H == (int)COOP_MAX_H, "tcv_coop_policy.h states the kernel's limit");
static int g_solver_variant = 0;   // 0: chain layout when the graph allows it, 1: always the dense 171-dim layout
int tcv::solver_variant() { return g_solver_variant; }
static int g_coop_helpers = -1;    // cooperative mode of small batches: -1 automatic, 0 off, h >= 1: h helper workgroups per window (when the batch allows it)
extern "C" int tcv_set_solver_variant(int variant) {
    if (variant != 0 && variant != 1) return TCV_ERR_INVALID;
    g_solver_variant = variant;
    return TCV_OK;
}
extern "C" int tcv_set_cooperative(int helpers) {
    if (helpers < -1 || helpers > COOP_MAX_H) { set_error("set_cooperative: -1 (automatic), 0 (off) or 1..7 helper workgroups per window"); return TCV_ERR_INVALID; }
    g_coop_helpers = helpers;
    return TCV_OK;
}

// =====================================================================================================
// batch: many independent windows resident in HBM
// =====================================================================================================
void tcv::BatchMemory::release() {
    tcv::dev_free(d_input);      // (d_dpool, d_win, d_plans, d_plan_base, d_ipool point into it)
    tcv::dev_free(d_imublk); tcv::dev_free(d_spill); tcv::dev_free(d_sqrt_out);
    tcv::dev_free(d_zero); tcv::dev_free(d_state);      // (d_delta, d_scratch, d_summary, d_prof live inside d_zero)
    *this = BatchMemory();
}
void tcv::CoopPlan::release() {
    tcv::dev_free(d_ctl); tcv::dev_free(d_x); tcv::dev_free(d_exp);
    d_ctl = nullptr; d_x = d_exp = nullptr;
}
void tcv::BatchFlight::release() {
    if (ev_order) (void)hipEventDestroy(ev_order);
    if (ev_inflight) (void)hipEventDestroy(ev_inflight);
    ev_order = ev_inflight = nullptr;
}
void tcv::StateDownload::release() {
    if (dl_staging) { if (ev_dl) (void)hipEventSynchronize(ev_dl); tcv::host_staging_release(dl_staging); dl_staging = nullptr; }
    if (ev_dl) (void)hipEventDestroy(ev_dl);
    ev_dl = nullptr;
}
void tcv::LastSolve::release() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
}
// The one release order of a batch.  The buffers go back to pools that other host threads take from, so nothing of this batch may still be
// running on any stream it used when the first of them is released: the waits come first, the side states (whose buffers the same work
// reads and writes) last.
static void batch_free(tcv_batch *b) {
    if (!b) return;
    (void)b->flight.wait_all();      // the event in flight, every stream
    b->dl.release();                 // the download staging, behind its event
    b->flight.release();             // the events
    tcv::coop_release(b->shape.dev, &b->claim);      // the cooperative claim (solve_finished without the duration: nobody is left to read it)
    b->mem.release();                // the device buffers
    b->coop.release();
    b->last.release();
    b->marg.reset(); b->eval.reset(); b->cov.reset(); b->relo.reset();      // the side states
    delete b;
}

// (a plan out of the cache carries the hash of its template, computed once by the thread that built it)
static unsigned long long plan_hash_of(const Packed &pk) { return pk.tmpl ? pk.tmpl->hash : tcv::plan_content_hash(pk.hdr, pk.ints); }
// The plan and the data size of every window under the batch's policy: chain or dense layout (b->shape.chain), LDS doubles of a chain-layout
// workgroup (b->shape.chain_lds), cooperative helpers per window (b->coop.h).  A fall-back rewrites the policy and packs the batch again.
// packing (symbolic elimination, gather programs, data layout) is independent per window: host threads share the work
static int pack_plans(tcv_batch *b, const tcv::HostOp &host_op) {
    auto pack_all = [&]() -> int {
        const int mode = b->shape.chain ? 0 : 1;
        const int nth = host_op.threads(std::min(b->in.n, 16));
        PackErrors err(b->in.n, nth);
        tcv::parallel_items(b->in.n, nth, [&](int w, int t) {
            const int rc = pack_problem(*b->in.problems[w], b->in.packed[w], nullptr, mode, b->shape.chain_lds, true, b->coop.h);      // plan + data size
            err.note(w, t, rc);
            // hash of the plan for the structure de-duplication below (a plan out of the cache is de-duplicated by its template: hashed
            // there, once per template, not once per window)
            if (rc == TCV_OK && !b->in.packed[w].tmpl && !b->in.packed[w].key_hashed) b->in.packed[w].plan_hash = plan_hash_of(b->in.packed[w]);
        });
        return err.first();
    };
    int rc = pack_all();
    // a window that does not fit half a CU's LDS (more than ~280 landmarks: its vectors over the unknowns and the chain's working set leave no
    // pool for the visual chunks) gives the WHOLE batch one workgroup per CU with all 160 KiB -- up to 1024 landmarks / 4096 point factors --
    // instead of failing; such a batch runs at 1 / 1.7 of the two-per-CU rate
    if (rc == TCV_ERR_TOO_LARGE && b->shape.chain && b->shape.chain_lds < (int)LDS_DOUBLES && !getenv("TCV_CHAIN_LDS_DOUBLES")) {
        b->shape.chain_lds = (int)LDS_DOUBLES;
        rc = pack_all();
    }
    if (rc == TCV_OK && b->coop.h > 0)
        for (int w = 0; w < b->in.n; w++) {      // what the cooperative master assumes: the prior staged in one piece, one IMU chunk
            const PlanHdr &H = b->in.packed[w].hdr;
            if (!H.chain || H.n_imu_chunk > 1 || H.camw != (int)CAM_W || (H.prior_n > 0 && H.prior_n * H.prior_n + 2 * H.prior_n > H.c_stage_cap)) {      // (the export layout of the helpers holds CAM_W-wide vectors)
                b->coop.h = 0;
                rc = pack_all();
                break;
            }
        }
    if (rc == TCV_OK && b->shape.chain)
        for (int w = 0; w < b->in.n; w++)
            if (!b->in.packed[w].hdr.chain) {      // a window is not chain-eligible: the whole batch uses the dense layout
                b->shape.chain = false; b->coop.h = 0;
                rc = pack_all();
                break;
            }
    return rc;
}
// the distinct plans of the batch and what the windows' sizes add up to
struct PlanSet {
    std::vector<std::pair<const int *, size_t>> src;      // per device plan: its ints on the host
    size_t ipool_size = 0, dtotal = 0;
};
// structure de-duplication (b->in.plans, b->in.plan_base, WinHdr::plan), the windows' offsets in the data pool (WinHdr::dbase) and what the
// largest window asks of the batch (strides, LDS, spill and coupling stores)
static void dedup_plans(tcv_batch *b, PlanSet &ps) {
    std::unordered_map<unsigned long long, std::vector<int>> plan_by_hash;
    std::map<const PlanTemplate *, int> plan_of_tmpl;   // windows that share a cached plan template share the device plan
    for (int w = 0; w < b->in.n; w++) {
        Packed &pk = b->in.packed[w];
        const PlanInts &pints = pk.tmpl ? pk.tmpl->ints : pk.ints;
        int pid = -1;
        if (pk.tmpl) { auto it = plan_of_tmpl.find(pk.tmpl.get()); if (it != plan_of_tmpl.end()) pid = it->second; }
        if (pid < 0) {
            // equal plans share one device copy: candidates by hash (computed with the packing, in parallel), confirmed by comparison -- the
            // replay's windows are all different (200 KB of plan each), the benchmark's all equal
            if (pk.tmpl) pk.plan_hash = plan_hash_of(pk);
            std::vector<int> &cands = plan_by_hash[pk.plan_hash];
            for (int c : cands)
                if (ps.src[c].second == pints.size() && std::memcmp(&b->in.plans[c], &pk.hdr, sizeof(PlanHdr)) == 0 &&
                    std::memcmp(ps.src[c].first, pints.data(), sizeof(int) * pints.size()) == 0) { pid = c; break; }
            if (pid < 0) {
                pid = (int)b->in.plans.size();
                cands.push_back(pid);
                b->in.plans.push_back(pk.hdr);
                b->in.plan_base.push_back((long long)ps.ipool_size);
                ps.src.push_back({pints.data(), pints.size()});      // (stays valid: pk.ints / the template live until the copy into the staging buffer)
                ps.ipool_size += pints.size();
            }
            if (pk.tmpl) plan_of_tmpl[pk.tmpl.get()] = pid;
        }
        pk.win.plan = pid;
        pk.win.dbase = (long long)ps.dtotal;
        ps.dtotal += (size_t)pk.win.n_doubles;
        b->in.state_stride = std::max(b->in.state_stride, (pk.hdr.nx + pk.hdr.nland + 1) & ~1);
        b->in.delta_stride = std::max(b->in.delta_stride, (pk.hdr.nc + pk.hdr.nland + 1) & ~1);
        const int nt = pk.hdr.nt;
        const size_t lds = b->shape.chain ? (size_t)b->shape.chain_lds * 8
                                    : (size_t)(nt * (nt + 1) / 2 * 256 + 2 * ((pk.hdr.nx + pk.hdr.nland + 1) & ~1) + (3 * pk.hdr.camw + 176) + 64 + pk.hdr.lds_area) * 8;
        b->shape.lds_bytes = std::max(b->shape.lds_bytes, lds);
        b->shape.spill_stride = std::max(b->shape.spill_stride, pk.hdr.c_spill);
        b->shape.hcl_cap = std::max(b->shape.hcl_cap, (pk.hdr.hcl_total + 63) & ~63);
        b->in.input_bytes += 8.0 * pk.win.n_doubles;
    }
    b->in.plan_bytes = 4.0 * ps.ipool_size;
}
// ONE pinned staging buffer and ONE device blob for everything the kernels read: [data pool | window headers | plan headers | plan
// offsets | plan ints | splice jobs], one asynchronous copy on the calling thread's own stream (five synchronous copies through the default
// stream used to cost a lock-step frame more than its packing)
// device-resident priors (tcv_batch_get_priors_device): nothing of them is packed or uploaded.  Their J0 | r0 | x0 regions live in a
// device-only tail behind the uploaded blob (WinHdr::d_prior is relative to the window's slice and simply points there), filled by one
// splice job per window on the upload's stream
struct BlobLayout {
    size_t o_win, o_plans, o_pbase, o_ipool, o_jobs, in_bytes, dev_bytes;      // byte offsets; uploaded bytes; with the device-only tail
    size_t n_jobs = 0;
    std::vector<int> splice_win, splice_imu_win;      // windows with a device-resident prior / with device-resident IMU factors
    std::vector<long long> tail_off, tail_imu;        // their regions in the tail (doubles)
};
static BlobLayout blob_layout(const tcv_batch *b, const PlanSet &ps) {
    const int n = b->in.n;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    BlobLayout L;
    L.o_win = up16(sizeof(double) * std::max<size_t>(1, ps.dtotal)); L.o_plans = up16(L.o_win + sizeof(WinHdr) * (size_t)n);
    L.o_pbase = up16(L.o_plans + sizeof(PlanHdr) * b->in.plans.size()); L.o_ipool = up16(L.o_pbase + sizeof(long long) * b->in.plan_base.size());
    L.tail_off.assign(n, -1); L.tail_imu.assign(n, -1);
    size_t tail_doubles = 0;
    for (int w = 0; w < n; w++) {
        if (b->in.packed[w].dev_prior_doubles > 0) { L.splice_win.push_back(w); L.tail_off[w] = (long long)tail_doubles; tail_doubles += ((size_t)b->in.packed[w].dev_prior_doubles + 1) & ~(size_t)1; L.n_jobs++; }
        if (b->in.packed[w].dev_imu_doubles > 0) { L.splice_imu_win.push_back(w); L.tail_imu[w] = (long long)tail_doubles; tail_doubles += ((size_t)b->in.packed[w].dev_imu_doubles + 1) & ~(size_t)1; L.n_jobs += b->in.problems[w]->imu.size(); }
    }
    L.o_jobs = up16(L.o_ipool + sizeof(int) * std::max<size_t>(1, ps.ipool_size));
    L.in_bytes = up16(L.o_jobs + sizeof(PriorSplice) * L.n_jobs);
    L.dev_bytes = L.in_bytes + sizeof(double) * tail_doubles;
    return L;
}
// data half: every window written straight into the pinned upload buffer, in parallel, and the plans' ints beside them; then the window
// headers of the batch (b->in.wins)
static int pack_data(tcv_batch *b, const tcv::HostOp &host_op, const PlanSet &ps, const BlobLayout &L, double *h_dpool) {
    const int n = b->in.n, n_plans = (int)ps.src.size();
    const int nth = host_op.threads(std::min(n, 16));
    PackErrors err(n, nth);
    tcv::parallel_items(n + n_plans, nth, [&](int i, int t) {
        if (i < n_plans) {      // the plans straight into the upload buffer (the larger items first)
            std::memcpy((char *)h_dpool + L.o_ipool + sizeof(int) * (size_t)b->in.plan_base[i], ps.src[i].first, sizeof(int) * ps.src[i].second);
            return;
        }
        const int w = i - n_plans;
        err.note(w, t, pack_problem_data(*b->in.problems[w], b->in.packed[w], nullptr, h_dpool + b->in.packed[w].win.dbase));
    });
    for (int w = 0; w < n; w++) { b->in.packed[w].ints.clear(); b->in.packed[w].ints.shrink_to_fit(); }
    if (int rc = err.first()) return rc;
    const long long tail = (long long)(L.in_bytes / sizeof(double));
    // the prior region of the window: in the tail, addressed relative to the window's own slice; likewise the constants of its (device-resident) IMU factors
    for (int w : L.splice_win) b->in.packed[w].win.d_prior = (int)(tail + L.tail_off[w] - b->in.packed[w].win.dbase);
    for (int w : L.splice_imu_win) b->in.packed[w].win.d_imu = (int)(tail + L.tail_imu[w] - b->in.packed[w].win.dbase);
    for (int w = 0; w < n; w++) b->in.wins.push_back(b->in.packed[w].win);
    return TCV_OK;
}
// the launch shape of the solve: one workgroup per window, or the cooperative groups with the whole LDS each
static void set_launch_shape(tcv_batch *b, int n_cu) {
    const int n = b->in.n;
    b->shape.grid = std::min(n, n_cu * ((b->shape.chain && b->shape.chain_lds < (int)LDS_DOUBLES) ? 2 : 1));      // (two workgroups per CU only when each takes half its LDS)
    if (const char *eg = getenv("TCV_GRID")) { const int g = atoi(eg); if (g > 0) b->shape.grid = std::min(n, g); }      // tuning experiments
    b->shape.slots = b->shape.grid;
    // ESTIMATE_TD windows: the kernel instance with ProjectionTdFactor.  It also takes the windows with a relocalisation pose (camera vectors 184
    // wide, PlanHdr::camw): the width is a literal in the instance every shipped configuration runs (build.py: -DTCV_CAMW_CONST for that
    // translation unit; read from the plan it cost the benchmark 0.3 %), a plan field in this one
    if (b->shape.chain) for (const Packed &pk : b->in.packed) if ((pk.hdr.flags & 1) || pk.hdr.camw != (int)CAM_W) { b->shape.chain_td = true; break; }
    if (b->coop.h > 0) {
        b->coop.groups = std::min(n, 8 * std::max(1, (n_cu / 8) / (1 + b->coop.h)));      // whole groups per XCD
        b->shape.slots = b->coop.groups;
        b->shape.grid = (1 + b->coop.h) * ((b->coop.groups + 7) & ~7);
        b->shape.lds_bytes = (size_t)LDS_DOUBLES * 8;
        int te_max = 0;
        for (auto &H : b->in.plans) { b->coop.exp_chunks = std::max(b->coop.exp_chunks, H.n_vis_chunk); te_max = std::max(te_max, (H.nt_c * (H.nt_c + 1) / 2) << 8); }
        b->coop.exp_stride = 2 * te_max + COOP_EXP_VEC;
    }
}
// window headers, plan headers, plan offsets and the splice jobs into the upload buffer `hb` (the data pool and the plan ints are there)
static void write_headers_and_jobs(const tcv_batch *b, const BlobLayout &L, char *hb) {
    const std::vector<tcv_problem *> &problems = b->in.problems;
    std::memcpy(hb + L.o_win, b->in.wins.data(), sizeof(WinHdr) * (size_t)b->in.n);
    std::memcpy(hb + L.o_plans, b->in.plans.data(), sizeof(PlanHdr) * b->in.plans.size());
    std::memcpy(hb + L.o_pbase, b->in.plan_base.data(), sizeof(long long) * b->in.plan_base.size());
    PriorSplice *hj = (PriorSplice *)(hb + L.o_jobs);
    for (size_t q = 0; q < L.splice_win.size(); q++) {
        const int w = L.splice_win[q];
        const tcv_prior *pr = problems[w]->prior[0].prior;
        PriorSplice &J = hj[q];
        std::memset(&J, 0, sizeof J);
        J.src = pr->d_block; J.dst = b->in.packed[w].win.dbase + b->in.packed[w].win.d_prior;
        J.n = pr->n; J.k0 = b->in.packed[w].win.prior_k0; J.nblk = (int)pr->size.size();
        J.k0_src = b->in.packed[w].prior_k0_deferred ? pr->d_k0 : nullptr; J.win = w;
        for (int k = 0; k < J.nblk; k++) { J.goff[k] = pr->x_goff[k]; J.size[k] = pr->size[k]; }
    }
    size_t q = L.splice_win.size();
    for (int w : L.splice_imu_win)
        for (size_t f = 0; f < problems[w]->imu.size(); f++, q++) {
            PriorSplice &J = hj[q];
            std::memset(&J, 0, sizeof J);
            J.kind = 1; J.src = problems[w]->imu[f].dev->d_out;
            J.dst = b->in.packed[w].win.dbase + b->in.packed[w].win.d_imu + (long long)f * IMU_CONST;
        }
}
// the device blob, its upload from `up.host` and, behind it on the same stream, the splice of the device-resident inputs
static int upload_and_splice(tcv_batch *b, const BlobLayout &L, tcv::StagedTransfer &up) {
    const std::vector<tcv_problem *> &problems = b->in.problems;
    hipError_t e_ = up.dev_alloc(L.dev_bytes);
    if (e_ == hipSuccess) e_ = hipMemcpyAsync(up.dev, up.host, L.in_bytes, hipMemcpyHostToDevice, up.st);
    if (e_ != hipSuccess) return hip_fail(e_, "upload of the batch");
    char *db = (char *)up.dev;
    b->mem.d_dpool = (double *)db; b->mem.d_win = (WinHdr *)(db + L.o_win); b->mem.d_plans = (PlanHdr *)(db + L.o_plans);
    b->mem.d_plan_base = (long long *)(db + L.o_pbase); b->mem.d_ipool = (int *)(db + L.o_ipool);
    // the splice jobs (if any) behind the upload on its stream; a source whose producer did not wait for its kernel carries an event
    for (int w : L.splice_imu_win)
        for (size_t f = 0; f < problems[w]->imu.size(); f++)
            if (const int rcw = problems[w]->imu[f].dev->dev->wait_ready(up.st)) return rcw;
    for (int w : L.splice_win)
        if (const int rcw = problems[w]->prior[0].prior->dev->wait_ready(up.st)) return rcw;
    return tcv::launch_prior_splice((const PriorSplice *)(db + L.o_jobs), (int)L.n_jobs, b->mem.d_dpool, (void *)b->mem.d_win, up.st);
}
// a pooled device buffer of cnt (at least one) T
template <class T> static hipError_t dev_array(T *&dst, size_t cnt) { return tcv::dev_malloc((void **)&dst, sizeof(T) * std::max<size_t>(1, cnt)); }
// the buffers the kernels write; *zero_bytes: size of the block that starts as zeros (b->mem.d_zero)
static hipError_t alloc_work_buffers(tcv_batch *b, size_t *zero_bytes) {
    const int n = b->in.n, scr = tcv_solve_scratch_doubles() + b->shape.hcl_cap;
    hipError_t e_ = dev_array(b->mem.d_state, (size_t)n * b->in.state_stride);
    if (e_ != hipSuccess) return e_;
    // the four buffers that start as zeros share ONE allocation and one memset: four fill kernels of 4 - 5 us with their launch gaps sat between
    // the upload and the frame's solve (a lock-step frame's GPU timeline, tools/gpu_calls.md#r05_gpu_z43: ~50 us of a 2.1 ms frame)
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_delta = 0, o_scr = up256(o_delta + sizeof(double) * std::max<size_t>(1, (size_t)n * b->in.delta_stride));
    const size_t o_sum = up256(o_scr + sizeof(double) * std::max<size_t>(1, (size_t)b->shape.slots * scr));
    const size_t o_prof = up256(o_sum + sizeof(DevSummary) * std::max<size_t>(1, (size_t)n));
    *zero_bytes = up256(o_prof + sizeof(double) * std::max<size_t>(1, (size_t)32 * b->shape.slots));
    if ((e_ = tcv::dev_malloc(&b->mem.d_zero, *zero_bytes)) != hipSuccess) return e_;
    char *z = (char *)b->mem.d_zero;
    b->mem.d_delta = (double *)(z + o_delta); b->mem.d_scratch = (double *)(z + o_scr); b->mem.d_summary = (DevSummary *)(z + o_sum); b->mem.d_prof = (double *)(z + o_prof);
    const bool coop = b->coop.h > 0;
    if (b->shape.chain) e_ = dev_array(b->mem.d_imublk, (size_t)b->shape.slots * 16 * IMU_BLK);
    if (b->shape.chain && e_ == hipSuccess) e_ = dev_array(b->mem.d_spill, (size_t)b->shape.slots * b->shape.spill_stride);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->coop.d_ctl, (size_t)b->coop.groups * COOP_CTL_INTS);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->coop.d_x, (size_t)b->coop.groups * COOP_X_DOUBLES);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->coop.d_exp, (size_t)b->coop.groups * b->coop.exp_chunks * b->coop.exp_stride);
    return e_;
}

extern "C" int tcv_batch_create(tcv_batch **out, tcv_problem *const *problems, tcv_problem *const *marg_problems,
                                double *const *const *marg_drop, const int *marg_num_drop, int n) {
    if (!out || !problems || n <= 0) { set_error("batch_create: bad argument"); return TCV_ERR_INVALID; }
    for (int w = 0; w < n; w++)
        if (!problems[w] || (marg_problems && (!marg_drop || !marg_num_drop))) { set_error("batch_create: null problem in the batch"); return TCV_ERR_INVALID; }
    if (int rc = device_ready()) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    tcv::prior_refresh_switch();
    const tcv::HostOp host_op;      // host threads of this call: the granted cores shared with the batch-level calls running beside it
    tcv_batch *b = new tcv_batch();
    std::unique_ptr<tcv_batch, void (*)(tcv_batch *)> owner(b, batch_free);      // every error exit frees the batch -- behind the upload guard's wait below
    b->in.n = n;
    b->in.problems.assign(problems, problems + n);
    b->in.packed.resize(n);
    { int cur = -1; if (hipGetDevice(&cur) != hipSuccess) cur = -1; for (auto &pk : b->in.packed) pk.batch_dev = cur; }
    int dev = 0, n_cu = 0;
    hipError_t e0 = hipGetDevice(&dev);
    if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e0 != hipSuccess) return hip_fail(e0, "hipDeviceGetAttribute");
    if (n_cu <= 0) n_cu = 256;
    b->shape.n_cu = n_cu; b->shape.dev = dev;
    // the chain layout is used only if every window of the batch allows it: the packing pass below starts over with the dense layout
    // at the first window that does not
    b->shape.chain = g_solver_variant == 0;
    // chain layout: two workgroups share a CU's LDS when the batch is larger than the chip; a batch that leaves CUs idle anyway gives
    // every workgroup the whole 160 KiB (fewer chunk passes over the visual factors, the prior's J0 staged in one piece)
    b->shape.chain_lds = (n <= n_cu && !getenv("TCV_CHAIN_LDS_DOUBLES")) ? (int)LDS_DOUBLES : chain_lds_doubles();
    size_t fmax = 0;
    for (int w = 0; w < n; w++) fmax = std::max(fmax, problems[w]->proj.size() + problems[w]->line.size());
    if (b->shape.chain) {      // the request: tcv_set_cooperative, overridden by TCV_COOP_H
        const bool automatic = g_coop_helpers < 0 && !getenv("TCV_COOP_H");
        int want = g_coop_helpers;
        if (const char *eh = getenv("TCV_COOP_H")) want = atoi(eh);
        b->coop.h = coop_helper_count(n, fmax, n_cu, want, automatic);
    }
    if (int rc = pack_plans(b, host_op)) return rc;
    const auto t_plans = std::chrono::steady_clock::now();
    PlanSet ps;
    dedup_plans(b, ps);
    const BlobLayout L = blob_layout(b, ps);
    if (L.dev_bytes / sizeof(double) >= ((size_t)1 << 31)) { set_error("batch too large (data pool offsets are 32-bit)"); return TCV_ERR_TOO_LARGE; }
    hipStream_t ust = tcv::util_stream();
    auto t_dedup = t_plans, t_packed = t_plans, t_marg = t_plans, t_issue = t_plans, t_alloc = t_plans;
    {
        tcv::StagedTransfer up(ust, L.in_bytes);      // the pinned upload buffer; the device blob until the batch takes it over
        if (!up.host) { set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
        t_dedup = std::chrono::steady_clock::now();
        if (int rc = pack_data(b, host_op, ps, L, (double *)up.host)) return rc;
        t_packed = std::chrono::steady_clock::now();
        set_launch_shape(b, n_cu);
        // error exits from here on wait for the stream: tcv_marg_attach and the upload below put commands on it, and the asynchronous upload
        // may still be reading the pinned staging buffer and writing the device blob -- both go back to pools another host thread takes from
        up.issued();
        if (marg_problems) {      // the marginalisation problems first: which IMU factor's sqrt_info the solve exports is part of the window headers
            hipError_t e_ = tcv::dev_malloc((void **)&b->mem.d_sqrt_out, sizeof(double) * (size_t)n * 225);
            if (e_ != hipSuccess) return hip_fail(e_, "hipMalloc");
            if (int rc = tcv_marg_attach(b, marg_problems, marg_drop, marg_num_drop)) return rc;
            for (int w = 0; w < n; w++) b->in.wins[w].sqrt_export = tcv_marg_sqrt_source(b, w);
        }
        t_marg = std::chrono::steady_clock::now();
        write_headers_and_jobs(b, L, (char *)up.host);
        if (int rc = upload_and_splice(b, L, up)) return rc;
        t_issue = std::chrono::steady_clock::now();
        size_t zero_bytes = 0;
        if ((e0 = alloc_work_buffers(b, &zero_bytes)) != hipSuccess) return hip_fail(e0, "hipMalloc");
        t_alloc = std::chrono::steady_clock::now();
        e0 = hipMemsetAsync(b->mem.d_zero, 0, zero_bytes, ust);
        const int rc_relo = tcv_relo_attach(b, ust);      // (relocalisation windows: their table and record buffer; nothing otherwise)
        // the batch is complete on the device before any stream uses it (and the upload is drained before its staging buffer is released, whatever the memsets returned)
        const hipError_t es = up.wait();
        if (e0 == hipSuccess) e0 = es;
        b->mem.d_input = up.take_dev();      // (d_dpool, d_win, d_plans, d_plan_base, d_ipool point into it)
        if (rc_relo != TCV_OK) return rc_relo;
    }
    tcv::flush_deferred(ust);      // (this thread just waited for its stream)
    if (e0 != hipSuccess) return hip_fail(e0, "upload of the batch");
    e0 = hipEventCreate(&b->last.ev0);
    if (e0 == hipSuccess) e0 = hipEventCreate(&b->last.ev1);
    if (e0 != hipSuccess) return hip_fail(e0, "hipEventCreate");
    const auto t_up = std::chrono::steady_clock::now();
    if (getenv("TCV_DEBUG_PACK")) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) { return std::chrono::duration<double, std::milli>(c - a).count(); };
        fprintf(stderr, "[batch_create] n %d: plans %.3f ms, plan pool + staging %.3f ms, data %.3f ms\n", n, ms(t_begin, t_plans), ms(t_plans, t_dedup), ms(t_dedup, t_packed));
        fprintf(stderr, "[batch_create] n %d: pack %.3f ms, marg attach %.3f ms, blob + upload issue + splice %.3f ms, allocations %.3f ms, memsets + sync %.3f ms (%d splice jobs, %.1f KB up)\n", n,
                ms(t_begin, t_packed), ms(t_packed, t_marg), ms(t_marg, t_issue), ms(t_issue, t_alloc), ms(t_alloc, t_up), (int)L.n_jobs, L.in_bytes / 1024.0);
    }
    *out = owner.release();
    return TCV_OK;
}
// The marginalisation problems of a batch that was created without them: their packing and upload can then run while the batch's solve
// is on the device (the native estimator does: ~0.3 ms of a lock-step frame).  The solve of such a batch does not export an IMU factor's
// sqrt_info (which factor is part of the window headers, uploaded before): the marginalisation kernel forms its own -- same function, same bits.
extern "C" int tcv_batch_attach_marginalization(tcv_batch *b, tcv_problem *const *marg_problems, double *const *const *marg_drop, const int *marg_num_drop) {
    if (!b || !marg_problems || !marg_drop || !marg_num_drop) { set_error("batch_attach_marginalization: bad argument"); return TCV_ERR_INVALID; }
    if (b->marg) { set_error("batch_attach_marginalization: the batch has marginalisation problems already"); return TCV_ERR_INVALID; }
    const tcv::HostOp host_op;
    const int rc = tcv_marg_attach(b, marg_problems, marg_drop, marg_num_drop);
    if (rc != TCV_OK) b->marg.reset();      // (nothing half-attached stays behind)
    return rc;
}
extern "C" void tcv_batch_destroy(tcv_batch *b) { batch_free(b); }
extern "C" int tcv_batch_size(const tcv_batch *b) { return b ? b->in.n : 0; }
// a per-plan side table of the batch (tcv_host.h PlanTable): the evaluation's and the covariance's owner lists, the landmark slot tables
int tcv::plan_table_create(const tcv_batch *b, const std::function<int(int, std::vector<int> &)> &entry, const char *what_alloc, const char *what_upload, PlanTable *t) {
    const int np = (int)b->in.plans.size();
    std::vector<long long> base(np, -1);
    std::vector<int> ints, one;
    for (int w = 0; w < b->in.n; w++) {      // the first window of every distinct plan
        const int pl = b->in.wins[w].plan;
        if (base[pl] >= 0) continue;
        base[pl] = (long long)ints.size();
        if (int rc = entry(w, one)) return rc;
        ints.insert(ints.end(), one.begin(), one.end());
    }
    const size_t head = sizeof(long long) * (size_t)np, bytes = head + sizeof(int) * std::max<size_t>(1, ints.size());
    std::vector<char> img(bytes, 0);
    std::memcpy(img.data(), base.data(), head);
    if (!ints.empty()) std::memcpy(img.data() + head, ints.data(), sizeof(int) * ints.size());
    void *d = nullptr;
    if (hipError_t e = tcv::dev_malloc(&d, bytes)) return hip_fail(e, what_alloc);
    if (int rc = tcv::staged_upload(d, img.data(), bytes, what_upload)) { tcv::dev_free(d); return rc; }
    t->d = d; t->base = (long long *)d; t->ints = (int *)((char *)d + head);
    return TCV_OK;
}
