// C-ABI of include/tcv.h: the device-resident batch -- creation phase by phase, ceres::Solve, the marginalisation's entry points, the
// downloads, summaries and statistics -- with the admission of cooperative launches, and the single-problem conveniences tcv_solve and
// tcv_marginalize.  Host code only; there is no CPU fallback: without a HIP device every compute entry point returns TCV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "tcv_host.h"
#include "tcv_relo.h"      // RELO_REC: the relocalisation record that rides with the states

using namespace tcv;

extern "C" int tcv_launch_solve(const tcv::SolveArgs *args, int grid, int nthreads, size_t lds_bytes, void *stream);
extern "C" int tcv_solve_scratch_doubles(void);
static int g_solver_variant = 0;   // 0: chain layout when the graph allows it, 1: always the dense 171-dim layout
int tcv::solver_variant() { return g_solver_variant; }
// CUs claimed by cooperative launches in flight, per device AND per XCD: a cooperative kernel spins on its partners, so all cooperative
// grids in flight together must be resident (two half-resident cooperative kernels could wait for each other's CUs until their
// timeouts).  The members of a group share an XCD -- workgroup b of a launch is dispatched to XCD b % 8 and solve_kernel makes the
// members of group g the workgroups with b % 8 == (g + rot) % 8 -- so the budget that counts is the XCD's (n_cu / 8 CUs), not the
// chip's: five one-window batches of eight workgroups each, all starting at XCD 0, would pass a chip-wide count (40 of 256) and
// sit half-resident on that XCD's 32 CUs.  A launch therefore (1) rotates its groups so that its first group lands on the XCD with the
// fewest claimed CUs (SolveArgs::coop_rot) and (2) is admitted only if every XCD keeps its claims within its CUs.
static std::mutex g_coop_mu;
static int g_coop_claimed[64][8];
static void coop_release(tcv_batch *b) {
    if (b->coop_claim > 0) {
        std::lock_guard<std::mutex> g(g_coop_mu);
        for (int x = 0; x < 8; x++) g_coop_claimed[b->coop_dev & 63][x] -= b->coop_claim_xcd[x];
        b->coop_claim = 0;
    }
}
// admission of a cooperative launch of `groups` groups of `wg` workgroups each: fills b->coop_claim_xcd / coop_rot and returns true, or
// leaves the table untouched and returns false (the caller then runs the same plan on one workgroup per window: same bits)
static bool coop_admit(tcv_batch *b, int groups, int wg) {
    std::lock_guard<std::mutex> g(g_coop_mu);
    int *cl = g_coop_claimed[b->coop_dev & 63];
    const int per_xcd = std::max(1, b->n_cu / 8);
    int rot = 0;
    for (int x = 1; x < 8; x++) if (cl[x] < cl[rot]) rot = x;
    int need[8];
    for (int x = 0; x < 8; x++) need[x] = 0;
    for (int q = 0; q < 8; q++) need[(q + rot) & 7] = wg * ((groups + 7 - q) / 8);      // groups g = q, q + 8, ... land on XCD (q + rot) % 8
    for (int x = 0; x < 8; x++) if (cl[x] + need[x] > per_xcd) return false;
    int total = 0;
    for (int x = 0; x < 8; x++) { cl[x] += need[x]; b->coop_claim_xcd[x] = need[x]; total += need[x]; }
    b->coop_claim = total; b->coop_rot = rot;
    return true;
}
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
static void batch_free(tcv_batch *b) {
    if (!b) return;
    if (b->wait_inflight) (void)hipEventSynchronize(b->ev_inflight);
    if (b->pending)      // the buffers go back to the free list: nothing of this batch may still be running on any stream it used
        for (hipStream_t st : b->streams) { if (st) (void)hipStreamSynchronize(st); else (void)hipDeviceSynchronize(); }
    if (b->dl_staging) { if (b->ev_dl) (void)hipEventSynchronize(b->ev_dl); tcv::host_staging_release(b->dl_staging); b->dl_staging = nullptr; }
    if (b->ev_dl) (void)hipEventDestroy(b->ev_dl);
    if (b->ev_order) (void)hipEventDestroy(b->ev_order);
    if (b->ev_inflight) (void)hipEventDestroy(b->ev_inflight);
    coop_release(b);
    tcv::dev_free(b->d_input);      // (d_dpool, d_win, d_plans, d_plan_base, d_ipool point into it)
    tcv::dev_free(b->d_imublk); tcv::dev_free(b->d_spill); tcv::dev_free(b->d_sqrt_out);
    tcv::dev_free(b->d_coop_ctl); tcv::dev_free(b->d_coop_x); tcv::dev_free(b->d_coop_exp);
    if (b->d_relo) tcv::dev_free(b->d_relo);
    tcv::dev_free(b->d_zero); tcv::dev_free(b->d_state);      // (d_delta, d_scratch, d_summary, d_prof live inside d_zero)
    b->d_zero = nullptr; b->d_prof = nullptr; b->d_delta = nullptr; b->d_scratch = nullptr; b->d_summary = nullptr;
    if (b->ev0) hipEventDestroy(b->ev0);
    if (b->ev1) hipEventDestroy(b->ev1);
    if (b->marg_free) b->marg_free(b);
    tcv_eval_free(b);
    if (b->cov_free) b->cov_free(b);
    delete b;
}

// ---- tcv_batch_create, phase by phase ----------------------------------------------------------------------------------------
// Cooperative mode (tcv_packed.h COOP_*): a chain-layout batch that leaves most of the chip idle gives every window 1 + H workgroups.
// H: one helper per ~96 point / line factors of the largest window (`fmax` of them), as many as the CUs allow.  TCV_COOP_H overrides (0: off).
static int coop_helper_count(int n, size_t fmax, int n_cu) {
    const bool automatic = g_coop_helpers < 0 && !getenv("TCV_COOP_H");
    int want = g_coop_helpers;
    if (const char *eh = getenv("TCV_COOP_H")) want = atoi(eh);
    if (want < 0) want = fmax >= 96 ? std::min<int>(COOP_MAX_H, std::max<int>(2, (int)((fmax + 95) / 96))) : 0;
    want = std::min(want, (int)COOP_MAX_H);
    while (want > 0 && (long long)((n + 7) / 8) * (1 + want) > n_cu / 8) want--;      // the groups of a launch are dealt round-robin to the XCDs: per XCD ceil(n / 8) groups on n_cu / 8 CUs
    // A large batch seldom has the device to itself -- a lock-step replay drives it from two host threads, and a launch that fills the chip with
    // helpers makes the other thread's launch queue behind it (64 streams: 10.8 K windows/s with seven helpers per window against 12.1 K with
    // two; 128 streams: 15.5 K with three against 17.7 K with two; profiles/r05_replay_coop_helpers.txt).  From 24 windows on a launch takes
    // half the chip -- three quarters if that is what two helpers per window need; TCV_COOP_H / tcv_set_cooperative still decide otherwise.
    if (n >= 24 && automatic) {
        int w2 = want;
        while (w2 > 0 && (long long)n * (1 + w2) > n_cu / 2) w2--;
        if (w2 < 2 && want >= 2 && (long long)n * 3 <= (long long)n_cu * 3 / 4) w2 = 2;
        want = std::min(want, w2);
    }
    if (want == 1 && automatic) want = 0;      // a single helper is not worth the hand-offs
    return want;
}
// (a plan out of the cache carries the hash of its template, computed once by the thread that built it)
static unsigned long long plan_hash_of(const Packed &pk) { return pk.tmpl ? pk.tmpl->hash : tcv::plan_content_hash(pk.hdr, pk.ints); }
// The plan and the data size of every window under the batch's policy: chain or dense layout (b->chain), LDS doubles of a chain-layout
// workgroup (b->chain_lds), cooperative helpers per window (b->coop_h).  A fall-back rewrites the policy and packs the batch again.
// packing (symbolic elimination, gather programs, data layout) is independent per window: host threads share the work
static int pack_plans(tcv_batch *b, const tcv::HostOp &host_op) {
    auto pack_all = [&]() -> int {
        const int mode = b->chain ? 0 : 1;
        const int nth = host_op.threads(std::min(b->n, 16));
        PackErrors err(b->n, nth);
        tcv::parallel_items(b->n, nth, [&](int w, int t) {
            const int rc = pack_problem(*b->problems[w], b->packed[w], nullptr, mode, b->chain_lds, true, b->coop_h);      // plan + data size
            err.note(w, t, rc);
            // hash of the plan for the structure de-duplication below (a plan out of the cache is de-duplicated by its template: hashed
            // there, once per template, not once per window)
            if (rc == TCV_OK && !b->packed[w].tmpl && !b->packed[w].key_hashed) b->packed[w].plan_hash = plan_hash_of(b->packed[w]);
        });
        return err.first();
    };
    int rc = pack_all();
    // a window that does not fit half a CU's LDS (more than ~280 landmarks: its vectors over the unknowns and the chain's working set leave no
    // pool for the visual chunks) gives the WHOLE batch one workgroup per CU with all 160 KiB -- up to 1024 landmarks / 4096 point factors --
    // instead of failing; such a batch runs at 1 / 1.7 of the two-per-CU rate
    if (rc == TCV_ERR_TOO_LARGE && b->chain && b->chain_lds < (int)LDS_DOUBLES && !getenv("TCV_CHAIN_LDS_DOUBLES")) {
        b->chain_lds = (int)LDS_DOUBLES;
        rc = pack_all();
    }
    if (rc == TCV_OK && b->coop_h > 0)
        for (int w = 0; w < b->n; w++) {      // what the cooperative master assumes: the prior staged in one piece, one IMU chunk
            const PlanHdr &H = b->packed[w].hdr;
            if (!H.chain || H.n_imu_chunk > 1 || H.camw != (int)CAM_W || (H.prior_n > 0 && H.prior_n * H.prior_n + 2 * H.prior_n > H.c_stage_cap)) {      // (the export layout of the helpers holds CAM_W-wide vectors)
                b->coop_h = 0;
                rc = pack_all();
                break;
            }
        }
    if (rc == TCV_OK && b->chain)
        for (int w = 0; w < b->n; w++)
            if (!b->packed[w].hdr.chain) {      // a window is not chain-eligible: the whole batch uses the dense layout
                b->chain = false; b->coop_h = 0;
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
// structure de-duplication (b->plans, b->plan_base, WinHdr::plan), the windows' offsets in the data pool (WinHdr::dbase) and what the
// largest window asks of the batch (strides, LDS, spill and coupling stores)
static void dedup_plans(tcv_batch *b, PlanSet &ps) {
    std::unordered_map<unsigned long long, std::vector<int>> plan_by_hash;
    std::map<const PlanTemplate *, int> plan_of_tmpl;   // windows that share a cached plan template share the device plan
    for (int w = 0; w < b->n; w++) {
        Packed &pk = b->packed[w];
        const PlanInts &pints = pk.tmpl ? pk.tmpl->ints : pk.ints;
        int pid = -1;
        if (pk.tmpl) { auto it = plan_of_tmpl.find(pk.tmpl.get()); if (it != plan_of_tmpl.end()) pid = it->second; }
        if (pid < 0) {
            // equal plans share one device copy: candidates by hash (computed with the packing, in parallel), confirmed by comparison -- the
            // replay's windows are all different (200 KB of plan each), the benchmark's all equal
            if (pk.tmpl) pk.plan_hash = plan_hash_of(pk);
            std::vector<int> &cands = plan_by_hash[pk.plan_hash];
            for (int c : cands)
                if (ps.src[c].second == pints.size() && std::memcmp(&b->plans[c], &pk.hdr, sizeof(PlanHdr)) == 0 &&
                    std::memcmp(ps.src[c].first, pints.data(), sizeof(int) * pints.size()) == 0) { pid = c; break; }
            if (pid < 0) {
                pid = (int)b->plans.size();
                cands.push_back(pid);
                b->plans.push_back(pk.hdr);
                b->plan_base.push_back((long long)ps.ipool_size);
                ps.src.push_back({pints.data(), pints.size()});      // (stays valid: pk.ints / the template live until the copy into the staging buffer)
                ps.ipool_size += pints.size();
            }
            if (pk.tmpl) plan_of_tmpl[pk.tmpl.get()] = pid;
        }
        pk.win.plan = pid;
        pk.win.dbase = (long long)ps.dtotal;
        ps.dtotal += (size_t)pk.win.n_doubles;
        b->state_stride = std::max(b->state_stride, (pk.hdr.nx + pk.hdr.nland + 1) & ~1);
        b->delta_stride = std::max(b->delta_stride, (pk.hdr.nc + pk.hdr.nland + 1) & ~1);
        const int nt = pk.hdr.nt;
        const size_t lds = b->chain ? (size_t)b->chain_lds * 8
                                    : (size_t)(nt * (nt + 1) / 2 * 256 + 2 * ((pk.hdr.nx + pk.hdr.nland + 1) & ~1) + (3 * pk.hdr.camw + 176) + 64 + pk.hdr.lds_area) * 8;
        b->lds_bytes = std::max(b->lds_bytes, lds);
        b->spill_stride = std::max(b->spill_stride, pk.hdr.c_spill);
        b->hcl_cap = std::max(b->hcl_cap, (pk.hdr.hcl_total + 63) & ~63);
        b->input_bytes += 8.0 * pk.win.n_doubles;
    }
    b->plan_bytes = 4.0 * ps.ipool_size;
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
    const int n = b->n;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    BlobLayout L;
    L.o_win = up16(sizeof(double) * std::max<size_t>(1, ps.dtotal)); L.o_plans = up16(L.o_win + sizeof(WinHdr) * (size_t)n);
    L.o_pbase = up16(L.o_plans + sizeof(PlanHdr) * b->plans.size()); L.o_ipool = up16(L.o_pbase + sizeof(long long) * b->plan_base.size());
    L.tail_off.assign(n, -1); L.tail_imu.assign(n, -1);
    size_t tail_doubles = 0;
    for (int w = 0; w < n; w++) {
        if (b->packed[w].dev_prior_doubles > 0) { L.splice_win.push_back(w); L.tail_off[w] = (long long)tail_doubles; tail_doubles += ((size_t)b->packed[w].dev_prior_doubles + 1) & ~(size_t)1; L.n_jobs++; }
        if (b->packed[w].dev_imu_doubles > 0) { L.splice_imu_win.push_back(w); L.tail_imu[w] = (long long)tail_doubles; tail_doubles += ((size_t)b->packed[w].dev_imu_doubles + 1) & ~(size_t)1; L.n_jobs += b->problems[w]->imu.size(); }
    }
    L.o_jobs = up16(L.o_ipool + sizeof(int) * std::max<size_t>(1, ps.ipool_size));
    L.in_bytes = up16(L.o_jobs + sizeof(PriorSplice) * L.n_jobs);
    L.dev_bytes = L.in_bytes + sizeof(double) * tail_doubles;
    return L;
}
// data half: every window written straight into the pinned upload buffer, in parallel, and the plans' ints beside them; then the window
// headers of the batch (b->wins)
static int pack_data(tcv_batch *b, const tcv::HostOp &host_op, const PlanSet &ps, const BlobLayout &L, double *h_dpool) {
    const int n = b->n, n_plans = (int)ps.src.size();
    const int nth = host_op.threads(std::min(n, 16));
    PackErrors err(n, nth);
    tcv::parallel_items(n + n_plans, nth, [&](int i, int t) {
        if (i < n_plans) {      // the plans straight into the upload buffer (the larger items first)
            std::memcpy((char *)h_dpool + L.o_ipool + sizeof(int) * (size_t)b->plan_base[i], ps.src[i].first, sizeof(int) * ps.src[i].second);
            return;
        }
        const int w = i - n_plans;
        err.note(w, t, pack_problem_data(*b->problems[w], b->packed[w], nullptr, h_dpool + b->packed[w].win.dbase));
    });
    for (int w = 0; w < n; w++) { b->packed[w].ints.clear(); b->packed[w].ints.shrink_to_fit(); }
    if (int rc = err.first()) return rc;
    const long long tail = (long long)(L.in_bytes / sizeof(double));
    // the prior region of the window: in the tail, addressed relative to the window's own slice; likewise the constants of its (device-resident) IMU factors
    for (int w : L.splice_win) b->packed[w].win.d_prior = (int)(tail + L.tail_off[w] - b->packed[w].win.dbase);
    for (int w : L.splice_imu_win) b->packed[w].win.d_imu = (int)(tail + L.tail_imu[w] - b->packed[w].win.dbase);
    for (int w = 0; w < n; w++) b->wins.push_back(b->packed[w].win);
    return TCV_OK;
}
// the launch shape of the solve: one workgroup per window, or the cooperative groups with the whole LDS each
static void set_launch_shape(tcv_batch *b, int n_cu) {
    const int n = b->n;
    b->grid = std::min(n, n_cu * ((b->chain && b->chain_lds < (int)LDS_DOUBLES) ? 2 : 1));      // (two workgroups per CU only when each takes half its LDS)
    if (const char *eg = getenv("TCV_GRID")) { const int g = atoi(eg); if (g > 0) b->grid = std::min(n, g); }      // tuning experiments
    b->slots = b->grid;
    if (b->coop_h > 0) {
        b->coop_groups = std::min(n, 8 * std::max(1, (n_cu / 8) / (1 + b->coop_h)));      // whole groups per XCD
        b->slots = b->coop_groups;
        b->grid = (1 + b->coop_h) * ((b->coop_groups + 7) & ~7);
        b->lds_bytes = (size_t)LDS_DOUBLES * 8;
        int te_max = 0;
        for (auto &H : b->plans) { b->coop_exp_chunks = std::max(b->coop_exp_chunks, H.n_vis_chunk); te_max = std::max(te_max, (H.nt_c * (H.nt_c + 1) / 2) << 8); }
        b->coop_exp_stride = 2 * te_max + COOP_EXP_VEC;
    }
}
// window headers, plan headers, plan offsets and the splice jobs into the upload buffer `hb` (the data pool and the plan ints are there)
static void write_headers_and_jobs(const tcv_batch *b, const BlobLayout &L, char *hb) {
    const std::vector<tcv_problem *> &problems = b->problems;
    std::memcpy(hb + L.o_win, b->wins.data(), sizeof(WinHdr) * (size_t)b->n);
    std::memcpy(hb + L.o_plans, b->plans.data(), sizeof(PlanHdr) * b->plans.size());
    std::memcpy(hb + L.o_pbase, b->plan_base.data(), sizeof(long long) * b->plan_base.size());
    PriorSplice *hj = (PriorSplice *)(hb + L.o_jobs);
    for (size_t q = 0; q < L.splice_win.size(); q++) {
        const int w = L.splice_win[q];
        const tcv_prior *pr = problems[w]->prior[0].prior;
        PriorSplice &J = hj[q];
        std::memset(&J, 0, sizeof J);
        J.src = pr->d_block; J.dst = b->packed[w].win.dbase + b->packed[w].win.d_prior;
        J.n = pr->n; J.k0 = b->packed[w].win.prior_k0; J.nblk = (int)pr->size.size();
        J.k0_src = b->packed[w].prior_k0_deferred ? pr->d_k0 : nullptr; J.win = w;
        for (int k = 0; k < J.nblk; k++) { J.goff[k] = pr->x_goff[k]; J.size[k] = pr->size[k]; }
    }
    size_t q = L.splice_win.size();
    for (int w : L.splice_imu_win)
        for (size_t f = 0; f < problems[w]->imu.size(); f++, q++) {
            PriorSplice &J = hj[q];
            std::memset(&J, 0, sizeof J);
            J.kind = 1; J.src = problems[w]->imu[f].dev->d_out;
            J.dst = b->packed[w].win.dbase + b->packed[w].win.d_imu + (long long)f * IMU_CONST;
        }
}
// the device blob, its upload from `up.host` and, behind it on the same stream, the splice of the device-resident inputs
static int upload_and_splice(tcv_batch *b, const BlobLayout &L, tcv::StagedTransfer &up) {
    const std::vector<tcv_problem *> &problems = b->problems;
    hipError_t e_ = up.dev_alloc(L.dev_bytes);
    if (e_ == hipSuccess) e_ = hipMemcpyAsync(up.dev, up.host, L.in_bytes, hipMemcpyHostToDevice, up.st);
    if (e_ != hipSuccess) return hip_fail(e_, "upload of the batch");
    char *db = (char *)up.dev;
    b->d_dpool = (double *)db; b->d_win = (WinHdr *)(db + L.o_win); b->d_plans = (PlanHdr *)(db + L.o_plans);
    b->d_plan_base = (long long *)(db + L.o_pbase); b->d_ipool = (int *)(db + L.o_ipool);
    // the splice jobs (if any) behind the upload on its stream; a source whose producer did not wait for its kernel carries an event
    for (int w : L.splice_imu_win)
        for (size_t f = 0; f < problems[w]->imu.size(); f++)
            if (const int rcw = problems[w]->imu[f].dev->dev->wait_ready(up.st)) return rcw;
    for (int w : L.splice_win)
        if (const int rcw = problems[w]->prior[0].prior->dev->wait_ready(up.st)) return rcw;
    return tcv::launch_prior_splice((const PriorSplice *)(db + L.o_jobs), (int)L.n_jobs, b->d_dpool, (void *)b->d_win, up.st);
}
// a pooled device buffer of cnt (at least one) T
template <class T> static hipError_t dev_array(T *&dst, size_t cnt) { return tcv::dev_malloc((void **)&dst, sizeof(T) * std::max<size_t>(1, cnt)); }
// the buffers the kernels write; *zero_bytes: size of the block that starts as zeros (b->d_zero)
static hipError_t alloc_work_buffers(tcv_batch *b, size_t *zero_bytes) {
    const int n = b->n, scr = tcv_solve_scratch_doubles() + b->hcl_cap;
    hipError_t e_ = dev_array(b->d_state, (size_t)n * b->state_stride);
    if (e_ != hipSuccess) return e_;
    // the four buffers that start as zeros share ONE allocation and one memset: four fill kernels of 4 - 5 us with their launch gaps sat between
    // the upload and the frame's solve (a lock-step frame's GPU timeline, tools/gpu_calls.md#r05_gpu_z43: ~50 us of a 2.1 ms frame)
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_delta = 0, o_scr = up256(o_delta + sizeof(double) * std::max<size_t>(1, (size_t)n * b->delta_stride));
    const size_t o_sum = up256(o_scr + sizeof(double) * std::max<size_t>(1, (size_t)b->slots * scr));
    const size_t o_prof = up256(o_sum + sizeof(DevSummary) * std::max<size_t>(1, (size_t)n));
    *zero_bytes = up256(o_prof + sizeof(double) * std::max<size_t>(1, (size_t)32 * b->slots));
    if ((e_ = tcv::dev_malloc(&b->d_zero, *zero_bytes)) != hipSuccess) return e_;
    char *z = (char *)b->d_zero;
    b->d_delta = (double *)(z + o_delta); b->d_scratch = (double *)(z + o_scr); b->d_summary = (DevSummary *)(z + o_sum); b->d_prof = (double *)(z + o_prof);
    const bool coop = b->coop_h > 0;
    if (b->chain) e_ = dev_array(b->d_imublk, (size_t)b->slots * 16 * IMU_BLK);
    if (b->chain && e_ == hipSuccess) e_ = dev_array(b->d_spill, (size_t)b->slots * b->spill_stride);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->d_coop_ctl, (size_t)b->coop_groups * COOP_CTL_INTS);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->d_coop_x, (size_t)b->coop_groups * COOP_X_DOUBLES);
    if (coop && e_ == hipSuccess) e_ = dev_array(b->d_coop_exp, (size_t)b->coop_groups * b->coop_exp_chunks * b->coop_exp_stride);
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
    b->n = n;
    b->problems.assign(problems, problems + n);
    b->packed.resize(n);
    { int cur = -1; if (hipGetDevice(&cur) != hipSuccess) cur = -1; for (auto &pk : b->packed) pk.batch_dev = cur; }
    int dev = 0, n_cu = 0;
    hipError_t e0 = hipGetDevice(&dev);
    if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (e0 != hipSuccess) return hip_fail(e0, "hipDeviceGetAttribute");
    if (n_cu <= 0) n_cu = 256;
    b->n_cu = n_cu; b->coop_dev = dev;
    // the chain layout is used only if every window of the batch allows it: the packing pass below starts over with the dense layout
    // at the first window that does not
    b->chain = g_solver_variant == 0;
    // chain layout: two workgroups share a CU's LDS when the batch is larger than the chip; a batch that leaves CUs idle anyway gives
    // every workgroup the whole 160 KiB (fewer chunk passes over the visual factors, the prior's J0 staged in one piece)
    b->chain_lds = (n <= n_cu && !getenv("TCV_CHAIN_LDS_DOUBLES")) ? (int)LDS_DOUBLES : chain_lds_doubles();
    size_t fmax = 0;
    for (int w = 0; w < n; w++) fmax = std::max(fmax, problems[w]->proj.size() + problems[w]->line.size());
    if (b->chain) b->coop_h = coop_helper_count(n, fmax, n_cu);
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
            hipError_t e_ = tcv::dev_malloc((void **)&b->d_sqrt_out, sizeof(double) * (size_t)n * 225);
            if (e_ != hipSuccess) return hip_fail(e_, "hipMalloc");
            if (int rc = tcv_marg_attach(b, marg_problems, marg_drop, marg_num_drop)) return rc;
            for (int w = 0; w < n; w++) b->wins[w].sqrt_export = tcv_marg_sqrt_source(b, w);
        }
        t_marg = std::chrono::steady_clock::now();
        write_headers_and_jobs(b, L, (char *)up.host);
        if (int rc = upload_and_splice(b, L, up)) return rc;
        t_issue = std::chrono::steady_clock::now();
        size_t zero_bytes = 0;
        if ((e0 = alloc_work_buffers(b, &zero_bytes)) != hipSuccess) return hip_fail(e0, "hipMalloc");
        t_alloc = std::chrono::steady_clock::now();
        e0 = hipMemsetAsync(b->d_zero, 0, zero_bytes, ust);
        const int rc_relo = tcv_relo_attach(b, ust);      // (relocalisation windows: their table and record buffer; nothing otherwise)
        // the batch is complete on the device before any stream uses it (and the upload is drained before its staging buffer is released, whatever the memsets returned)
        const hipError_t es = up.wait();
        if (e0 == hipSuccess) e0 = es;
        b->d_input = up.take_dev();      // (d_dpool, d_win, d_plans, d_plan_base, d_ipool point into it)
        if (rc_relo != TCV_OK) return rc_relo;
    }
    tcv::flush_deferred(ust);      // (this thread just waited for its stream)
    if (e0 != hipSuccess) return hip_fail(e0, "upload of the batch");
    e0 = hipEventCreate(&b->ev0);
    if (e0 == hipSuccess) e0 = hipEventCreate(&b->ev1);
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
    if (rc != TCV_OK && b->marg && b->marg_free) b->marg_free(b);      // (nothing half-attached stays behind)
    return rc;
}
extern "C" void tcv_batch_destroy(tcv_batch *b) { batch_free(b); }
extern "C" int tcv_batch_size(const tcv_batch *b) { return b ? b->n : 0; }

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

int tcv_batch_enter_stream(tcv_batch *b, void *hip_stream) {
    hipStream_t st = (hipStream_t)hip_stream;
    if (b->wait_inflight) HIPCHK(hipStreamWaitEvent(st, b->ev_inflight, 0));      // (the stream that work ran on may be gone: its event orders the new call)
    else if (b->pending && b->last_stream != st) {
        if (!b->ev_order) HIPCHK(hipEventCreateWithFlags(&b->ev_order, hipEventDisableTiming));
        HIPCHK(hipEventRecord(b->ev_order, b->last_stream));
        HIPCHK(hipStreamWaitEvent(st, b->ev_order, 0));
    }
    if (std::find(b->streams.begin(), b->streams.end(), st) == b->streams.end()) b->streams.push_back(st);
    b->last_stream = st; b->pending = true;
    return TCV_OK;
}
// a per-plan side table of the batch (tcv_host.h PlanTable): the evaluation's and the covariance's owner lists, the landmark slot tables
int tcv::plan_table_create(const tcv_batch *b, const std::function<int(int, std::vector<int> &)> &entry, const char *what_alloc, const char *what_upload, PlanTable *t) {
    const int np = (int)b->plans.size();
    std::vector<long long> base(np, -1);
    std::vector<int> ints, one;
    for (int w = 0; w < b->n; w++) {      // the first window of every distinct plan
        const int pl = b->wins[w].plan;
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

static int wall_clock_khz() {
    int dev = 0, khz = 0;
    hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;      // 100 MHz on CDNA
    return khz;
}
extern "C" int tcv_batch_solve(tcv_batch *b, const tcv_solver_options *o, void *hip_stream) {
    if (!b || !o) return TCV_ERR_INVALID;
    if (hip_stream == TCV_STREAM_THREAD) hip_stream = (void *)tcv::util_stream();
    SolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->d_win; a.plans = b->d_plans; a.plan_base = b->d_plan_base; a.ipool = b->d_ipool; a.dpool = b->d_dpool;
    a.state_out = b->d_state; a.summary = b->d_summary; a.first_delta = o->record_first_step ? b->d_delta : nullptr;
    a.scratch = b->d_scratch;
    a.prof = b->d_prof;
    a.nwin = b->n; a.state_stride = b->state_stride; a.delta_stride = b->delta_stride; a.scratch_stride = tcv_solve_scratch_doubles() + b->hcl_cap;
    a.max_iterations = o->max_num_iterations; a.fixed_iterations = o->fixed_iterations; a.use_mfma = o->use_mfma;
    a.chain = b->chain ? 1 : 0; a.chain_td = 0;
    // ESTIMATE_TD windows: the kernel instance with ProjectionTdFactor.  It also takes the windows with a relocalisation pose (camera vectors 184
    // wide, PlanHdr::camw): the width is a literal in the instance every shipped configuration runs (build.py: -DTCV_CAMW_CONST for that
    // translation unit; read from the plan it cost the benchmark 0.3 %), a plan field in this one
    if (b->chain) for (int w = 0; w < b->n; w++) if ((b->packed[w].hdr.flags & 1) || b->packed[w].hdr.camw != (int)CAM_W) { a.chain_td = 1; break; }
    a.imublk = b->d_imublk; a.spill = b->d_spill; a.spill_stride = b->spill_stride;
    a.max_ticks = 0;
    a.sqrt_out = b->d_sqrt_out;
    // (a batch with a relocalisation window never fuses: double2vector's tail needs the un-fixed pose 0, tcv_relo.hip; the stand-alone kernel gives the same bits)
    a.gauge_fix = b->fuse_gauge && b->n_relo == 0 ? 1 : 0;
    // cooperative plans also run on the single-workgroup kernel (workgroups_per_window = 1): same chunks, same additions, same bits
    bool coop = b->coop_h > 0 && o->workgroups_per_window != 1;
    if (coop && b->coop_claim == 0)      // (a claim still held: the previous cooperative solve of this batch, same stream order, same rotation)
        if (!coop_admit(b, b->coop_groups, 1 + b->coop_h)) coop = false;      // the XCDs are taken by other cooperative launches: the same plan on one workgroup per window, the same bits
    const bool timed = o->max_solver_time_in_seconds > 0.0 && !o->fixed_iterations;
    const int khz = (coop || timed) ? wall_clock_khz() : 0;      // the cooperative time-out and the solver's time budget count its ticks
    int grid = b->grid;
    b->last_wg = coop ? 1 + b->coop_h : 1;
    if (coop) {
        a.coop_h = b->coop_h; a.coop_groups = b->coop_groups; a.coop_exp_chunks = b->coop_exp_chunks; a.coop_exp_stride = b->coop_exp_stride;
        a.coop_ctl = b->d_coop_ctl; a.coop_x = b->d_coop_x; a.coop_exp = b->d_coop_exp; a.coop_rot = b->coop_rot;
        a.coop_timeout = (long long)khz * 2000;      // 2 s
    } else if (b->coop_h > 0) grid = b->slots;
    b->sqrt_out_valid = b->d_sqrt_out != nullptr;
    if (const char *sk = getenv("TCV_ABLATE_SKIP")) a.pad2 = (int)(unsigned)strtoul(sk, nullptr, 0);      // -DTCV_ABLATE builds only read it
    if (timed) {
        a.max_ticks = (long long)(o->max_solver_time_in_seconds * 1e3 * (double)khz);
        if (a.max_ticks < 1) a.max_ticks = 1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = tcv_batch_enter_stream(b, hip_stream)) return rc;
    if (coop) HIPCHK(hipMemsetAsync(b->d_coop_ctl, 0, sizeof(int) * (size_t)b->coop_groups * COOP_CTL_INTS, st));
    HIPCHK(hipEventRecord(b->ev0, st));
    const int rc = tcv_launch_solve(&a, grid, (!b->chain && o->threads_per_window == 512) ? 512 : 256, b->lds_bytes, hip_stream);
    if (rc != 0) return hip_fail((hipError_t)rc, "solve kernel launch");
    HIPCHK(hipEventRecord(b->ev1, st));
    b->solved = true;
    b->relo_done = false;
    b->gauge_in_solve = a.gauge_fix != 0;
    if (a.gauge_fix) b->gauge_fixed = true;
    return TCV_OK;
}
extern "C" int tcv_batch_marginalize(tcv_batch *b, void *hip_stream) {
    if (!b) return TCV_ERR_INVALID;
    if (hip_stream == TCV_STREAM_THREAD) hip_stream = (void *)tcv::util_stream();
    if (int rc = tcv_batch_enter_stream(b, hip_stream)) return rc;
    return tcv_marg_run(b, hip_stream);
}
// waits for every stream this batch has work in flight on (the whole device when one of them is the default stream), not for the
// device: batches driven from different host threads on different streams overlap (bench.py --mode stream)
extern "C" int tcv_batch_synchronize(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (b->wait_inflight) { HIPCHK(hipEventSynchronize(b->ev_inflight)); b->wait_inflight = false; }
    for (hipStream_t st : b->streams) { if (st) HIPCHK(hipStreamSynchronize(st)); else HIPCHK(hipDeviceSynchronize()); }
    b->streams.clear();
    b->pending = false;
    coop_release(b);
    if (b->solved) hipEventElapsedTime(&b->solve_ms, b->ev0, b->ev1);
    tcv_marg_elapsed(b);
    return TCV_OK;
}
// the solved states (tcv_batch::h_state) into the callers' parameter blocks: camera blocks in plan order, then the inverse depths
static void scatter_states(const tcv_batch *b) {
    for (int w = 0; w < b->n; w++) {
        const Packed &pk = b->packed[w];
        const tcv_problem &p = *b->problems[w];
        const double *x = b->h_state.data() + (size_t)w * b->state_stride;
        int off = 0;
        for (int blk : pk.cam_block) { std::memcpy(p.blocks[blk].addr, x + off, sizeof(double) * p.blocks[blk].size); off += p.blocks[blk].size; }
        for (int blk : pk.lm_block) p.blocks[blk].addr[0] = x[off++];
    }
}
extern "C" int tcv_batch_download_states(tcv_batch *b) {
    if (!b || !b->solved) return TCV_ERR_INVALID;
    if (b->n_relo > 0) return tcv_batch_download_states_brief(b, nullptr, nullptr, nullptr);      // (the relocalisation records ride with the states, and their `valid` needs the terminations)
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    b->h_state.resize((size_t)b->n * b->state_stride);
    if (int rc = tcv::staged_download(b->h_state.data(), b->d_state, sizeof(double) * b->h_state.size(), "download of the states")) return rc;
    scatter_states(b);
    return TCV_OK;
}
// Split form for callers that enqueue more work behind the solve: _begin puts the copy of the states (and of the summary heads) on `hip_stream`
// behind whatever the batch has in flight there and returns; the caller may launch the marginalisation right behind it; _end waits for the
// COPY only (an event), not for the stream, and hands the results out.  The native estimator does: the marginalisation starts the moment the
// states have left, not a host round trip later.
extern "C" int tcv_batch_download_states_begin(tcv_batch *b, void *hip_stream) {
    if (!b || !b->solved) return TCV_ERR_INVALID;
    if (b->dl_staging) { set_error("batch_download_states_begin: a download is in flight already"); return TCV_ERR_INVALID; }
    if (hip_stream == TCV_STREAM_THREAD) hip_stream = (void *)tcv::util_stream();
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = tcv_batch_enter_stream(b, hip_stream)) return rc;
    b->h_state.resize((size_t)b->n * b->state_stride);
    const size_t sbytes = sizeof(double) * b->h_state.size(), hbytes = (size_t)32 * b->n;
    const bool relo = b->n_relo > 0 && b->relo_done;      // the relocalisation records of tcv_batch_gauge_fix (tcv_relo.hip) in the same round trip
    const size_t rbytes = relo ? sizeof(double) * (size_t)tcv::RELO_REC * b->n_relo : 0;
    static_assert(offsetof(DevSummary, final_cost) == 24 && offsetof(DevSummary, num_iterations) == 0 && offsetof(DevSummary, termination) == 4, "head of DevSummary");
    char *hs = (char *)host_staging_acquire(sbytes + hbytes + rbytes);
    if (!hs) { set_error("hipHostMalloc (download staging) failed"); return TCV_ERR_HIP; }
    hipError_t e_ = hipSuccess;
    if (!b->ev_dl) e_ = hipEventCreateWithFlags(&b->ev_dl, hipEventDisableTiming);
    if (e_ == hipSuccess) e_ = hipMemcpyAsync(hs, b->d_state, sbytes, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess) e_ = hipMemcpy2DAsync(hs + sbytes, 32, b->d_summary, sizeof(DevSummary), 32, (size_t)b->n, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess && relo) e_ = hipMemcpyAsync(hs + sbytes + hbytes, b->d_relo, rbytes, hipMemcpyDeviceToHost, st);
    if (e_ == hipSuccess) e_ = hipEventRecord(b->ev_dl, st);
    if (e_ != hipSuccess) { (void)tcv::stream_wait(st); host_staging_release(hs); return hip_fail(e_, "download of the states"); }
    b->dl_staging = hs;
    b->relo_in_dl = relo;
    return TCV_OK;
}
extern "C" int tcv_batch_download_states_end(tcv_batch *b, int *num_iterations, int *termination, double *final_cost) {
    if (!b || !b->dl_staging || !b->ev_dl) { set_error("batch_download_states_end: no download in flight"); return TCV_ERR_INVALID; }
    char *hs = (char *)b->dl_staging;
    const size_t sbytes = sizeof(double) * b->h_state.size();
    const hipError_t e_ = hipEventSynchronize(b->ev_dl);
    if (e_ == hipSuccess) {
        std::memcpy(b->h_state.data(), hs, sbytes);
        for (int w = 0; w < b->n; w++) {
            const char *q = hs + sbytes + (size_t)32 * w;
            int it, tm; double fc;
            std::memcpy(&it, q, 4); std::memcpy(&tm, q + 4, 4); std::memcpy(&fc, q + 24, 8);
            if (num_iterations) num_iterations[w] = it;
            if (termination) termination[w] = tm;
            if (final_cost) final_cost[w] = fc;
        }
        if (b->relo_in_dl) {
            b->h_relo.resize((size_t)tcv::RELO_REC * b->n_relo);
            std::memcpy(b->h_relo.data(), hs + sbytes + (size_t)32 * b->n, sizeof(double) * b->h_relo.size());
            b->relo_valid.assign(b->n_relo, 0);
            for (int k = 0; k < b->n_relo; k++) {
                int tm;
                std::memcpy(&tm, hs + sbytes + (size_t)32 * b->relo_win[k] + 4, 4);
                b->relo_valid[k] = tm != 5;      // FAILURE: the window's states are not a solution, neither is its record
            }
        }
        b->relo_have = b->relo_in_dl;
    }
    host_staging_release(hs);
    b->dl_staging = nullptr;
    if (e_ != hipSuccess) return hip_fail(e_, "download of the states");
    // the solve (and the gauge fix) lie behind the copy on the stream: they have finished -- its duration and the CUs its cooperative launch held
    coop_release(b);
    if (b->solved) (void)hipEventElapsedTime(&b->solve_ms, b->ev0, b->ev1);
    scatter_states(b);
    return TCV_OK;
}
// States into the callers' blocks AND the three numbers of the summary a per-frame caller reads (the reference reads one:
// summary.iterations.size(), estimator.cpp:1902) in ONE device round trip: the states and the heads of the summary records (32 of their
// 4 136 bytes, a pitched copy) on the calling thread's stream, one wait.
extern "C" int tcv_batch_download_states_brief(tcv_batch *b, int *num_iterations, int *termination, double *final_cost) {
    if (!b || !b->solved) return TCV_ERR_INVALID;
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
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
    if (!b || !out || n < 0 || n > b->n) { set_error("batch_get_summaries: n exceeds the batch size"); return TCV_ERR_INVALID; }
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    std::vector<DevSummary> h(n);
    if (int rc = tcv::staged_download(h.data(), b->d_summary, sizeof(DevSummary) * (size_t)n, "download of the summaries")) return rc;
    for (int i = 0; i < n; i++) summary_to_public(h[i], out + i);
    return TCV_OK;
}
// tangent step of iteration 1 in problem order: free camera blocks in the order they were added
// (local size each), then the inverse depths in landmark order.  Returns the length in *len.
extern "C" int tcv_batch_get_first_step(tcv_batch *b, int window, double *out, int cap, int *len) {
    if (!b || window < 0 || window >= b->n || !out) return TCV_ERR_INVALID;
    const PlanHdr &H = b->plans[b->wins[window].plan];
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;      // (like the other getters: the copy runs on the calling thread's stream, not behind the solve's)
    std::vector<double> d(b->delta_stride);
    if (int rc = tcv::staged_download(d.data(), b->d_delta + (size_t)window * b->delta_stride, sizeof(double) * b->delta_stride, "download of the first step")) return rc;
    const tcv_problem &p = *b->problems[window];
    const Packed &pk = b->packed[window];
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
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    return tcv_marg_get_prior(b, window, out);
}
extern "C" int tcv_batch_get_priors(tcv_batch *b, tcv_prior **out, int n) {
    if (!b || !out || n != b->n) { set_error("batch_get_priors: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    // (the per-window fallback of tcv_marg_get_prior copies on the stream of the thread that runs it, which is not ordered behind a
    // marginalisation launched on another stream: wait for the batch's own streams first)
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    const tcv::HostOp host_op;
    const int nth = host_op.threads(std::max(1, std::min(n / 16, 8)));
    std::vector<int> rcs(nth, TCV_OK);
    std::vector<std::string> msgs(nth);
    auto work = [&](int t) {
        // a worker thread starts on device 0: the batch's buffers live on its own device.  The CALLER runs this lambda too (parallel_run):
        // whatever thread it is, its current device is put back
        int prev = -1;
        if (nth > 1 && hipGetDevice(&prev) == hipSuccess && prev != b->coop_dev) (void)hipSetDevice(b->coop_dev); else prev = -1;
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
    if (!b || !out || n != b->n) { set_error("batch_get_priors_device_async: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    const int rc = tcv_marg_get_priors_device(b, out, n, true);      // (no wait: the marginalisation may still be running)
    if (rc == TCV_OK && b->pending && !b->streams.empty()) {
        // the batch outlives this call with work in flight: from here on that work is an event, not the streams it runs on -- the calling
        // thread may end (its stream goes with it) before somebody asks for the status or destroys the batch
        (void)tcv_marg_status_prefetch(b, (void *)b->last_stream);
        hipError_t e = hipSuccess;
        if (!b->ev_inflight) e = hipEventCreateWithFlags(&b->ev_inflight, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(b->ev_inflight, b->last_stream);
        if (e != hipSuccess) {
            // no event to track the work by: wait for it here (the streams are still this batch's) -- the handles stay valid, the call merely
            // was not asynchronous; if even that fails the handles are destroyed: "on an error out[] is all NULL" (include/tcv.h)
            const int rcs = tcv_batch_synchronize(b);
            if (rcs != TCV_OK) { for (int k = 0; k < n; k++) if (out[k]) { tcv_prior_destroy(out[k]); out[k] = nullptr; } return rcs; }
            return TCV_OK;
        }
        b->streams.clear();
        b->wait_inflight = true;
    }
    return rc;
}
extern "C" int tcv_batch_get_priors_device(tcv_batch *b, tcv_prior **out, int n) {
    if (!b || !out || n != b->n) { set_error("batch_get_priors_device: n must be the batch size"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n; k++) out[k] = nullptr;
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    return tcv_marg_get_priors_device(b, out, n, false);
}
extern "C" int tcv_batch_download_priors(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    return tcv_marg_download(b, 0);
}
extern "C" int tcv_batch_download_priors_compact(tcv_batch *b) {
    if (!b) return TCV_ERR_INVALID;
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) return rc;
    return tcv_marg_download(b, 1);
}
extern "C" int tcv_batch_stats(tcv_batch *b, double *input_bytes, double *solve_ms, double *marg_ms) {
    if (!b) return TCV_ERR_INVALID;
    if (input_bytes) *input_bytes = b->input_bytes;
    if (solve_ms) *solve_ms = b->solve_ms;
    if (marg_ms) *marg_ms = b->marg_ms;
    return TCV_OK;
}
// TCV_PROFILE builds only: copies (and clears) the 32 per-phase cycle accumulators of the solve kernel
extern "C" int tcv_batch_profile(tcv_batch *b, double *out32) {
    if (!b || !out32) return TCV_ERR_INVALID;
    std::vector<double> h((size_t)32 * b->slots);
    HIPCHK(hipMemcpy(h.data(), b->d_prof, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < 32; i++) { out32[i] = 0; for (int g = 0; g < b->slots; g++) out32[i] += h[(size_t)g * 32 + i]; }
    HIPCHK(hipMemset(b->d_prof, 0, sizeof(double) * h.size()));
    return TCV_OK;
}
extern "C" int tcv_batch_cooperative(const tcv_batch *b, int *helpers, int *groups, int *chunks, int *last_solve_workgroups) {
    if (!b) return TCV_ERR_INVALID;
    if (last_solve_workgroups) *last_solve_workgroups = b->last_wg;
    if (helpers) *helpers = b->coop_h;
    if (groups) *groups = b->coop_h > 0 ? b->coop_groups : 0;
    if (chunks) { int c = 0; for (auto &H : b->plans) c = std::max(c, H.n_vis_chunk); *chunks = c; }
    return TCV_OK;
}
// developer diagnostics: the control block of group `group` (COOP_CTL_INTS ints: request / served sequence numbers, abort flag, progress
// marks), copied on a private stream so that it can be read while a launch is still running
extern "C" int tcv_batch_debug_coop(tcv_batch *b, int group, int *out64) {
    if (!b || !out64 || b->coop_h <= 0 || group < 0 || group >= b->coop_groups) { set_error("debug_coop: no cooperative plan / bad group"); return TCV_ERR_INVALID; }
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipError_t e = hipMemcpyAsync(out64, b->d_coop_ctl + (size_t)group * COOP_CTL_INTS, sizeof(int) * COOP_CTL_INTS, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return hip_fail(e, "debug_coop copy");
    return TCV_OK;
}
extern "C" int tcv_batch_layout(const tcv_batch *b) { return b ? (b->chain ? 0 : 1) : TCV_ERR_INVALID; }
extern "C" int tcv_batch_plan_stats(tcv_batch *b, int *num_plans, double *plan_bytes, int *grid, int *lds_bytes) {
    if (!b) return TCV_ERR_INVALID;
    if (num_plans) *num_plans = (int)b->plans.size();
    if (plan_bytes) *plan_bytes = b->plan_bytes;
    if (grid) *grid = b->grid;
    if (lds_bytes) *lds_bytes = (int)b->lds_bytes;
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
