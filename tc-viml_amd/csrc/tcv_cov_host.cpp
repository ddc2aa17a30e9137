// Host half of the batched marginal covariance (include/tcv_covariance.h; the kernel: tcv_cov.hip): the request resolver, the owner
// lists of the reduced camera system S, the buffers of a batch and the getters; behind them the landmark call
// (include/tcv_landmark_covariance.h), which shares the owner lists and the work buffers and keeps result buffers of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>

#include "../../include/tcv_covariance.h"
#include "../../include/tcv_landmark_covariance.h"
#include "tcv_cov.h"
#include "tcv_host.h"

using namespace tcv;

extern "C" int tcv_launch_covariance(const tcv::CovArgs *args, int grid, size_t lds_bytes, void *stream);
extern "C" int tcv_launch_landmark_covariance(const tcv::CovArgs *args, int grid, size_t lds_bytes, void *stream);
namespace {
// the landmark call's half of a batch's covariance state (made at the first tcv_batch_compute_landmark_covariance)
struct LmState {
    void *d_tab = nullptr;      // [offset of every plan's slot table (long long) | the tables]
    void *d_ylm = nullptr;      // y_l of a chunk, per workgroup
    void *d_res = nullptr;      // [request tables | status | diagonal blocks of the cross requests | variances | cross rows] of the last cross list
    long long *d_tab_base = nullptr;
    int *d_tab_ints = nullptr;
    double *d_out = nullptr, *d_var = nullptr, *d_cross = nullptr;
    int *d_rq = nullptr, *d_status = nullptr;
    int lmax = 0, mstride = 0, rq_stride = 0;
    bool ready = false, have_req = false, computed = false;
    std::vector<tcv_landmark_cross_block> req;      // the last cross list
    std::vector<int> cols;                          // widths of its blocks
    std::vector<int> rq;                            // host copy of the request tables (first solved column of every block per window)
    std::vector<std::vector<int>> plan_of;          // per window: plan index of the l-th landmark in registration order
};
struct CovState {
    void *d_tab = nullptr;      // [offset of every plan's owner lists (long long) | the lists]
    void *d_work = nullptr;     // [staging | y] per workgroup
    void *d_res = nullptr;      // [request tables | status | blocks] of the last request list
    long long *d_tab_base = nullptr;
    int *d_tab_ints = nullptr;
    double *d_stage = nullptr, *d_y = nullptr, *d_out = nullptr;
    int *d_rq = nullptr, *d_status = nullptr;
    long long stage_stride = 0;
    int grid = 0, nc_max = 0;
    bool computed = false;
    std::vector<tcv_covariance_block> req;      // the last request list
    std::vector<int> rows, cols;                // sizes of its blocks
    LmState lm;
};
void cov_free(tcv_batch *b) {
    CovState *s = (CovState *)b->cov;
    if (!s) return;
    tcv::dev_free(s->d_tab); tcv::dev_free(s->d_work); tcv::dev_free(s->d_res);
    tcv::dev_free(s->lm.d_tab); tcv::dev_free(s->lm.d_ylm); tcv::dev_free(s->lm.d_res);
    delete s;
    b->cov = nullptr;
}
int block_width(const ParamBlock &pb) { return pb.kind == KIND_POSE ? 6 : pb.size; }

// the problem block of one half of a request; TCV_ERR_INVALID / TCV_ERR_UNSUPPORTED with the message set
int resolve(const tcv_problem &p, int kind, int index, int *blk, int *width) {
    auto frame = [&](const std::vector<int> &tab, const char *what) -> int {
        const int n = (int)tab.size();
        if (n == 0) { set_error(std::string("covariance: the window lacks a requested block: no frame table for ") + what + " (tcv_problem_set_frames)"); return -1; }
        const int i = index < 0 ? index + n : index;
        if (i < 0 || i >= n) { set_error(std::string("covariance: ") + what + " index out of range"); return -1; }
        if (tab[i] < 0) { set_error(std::string("covariance: the window lacks a requested block: ") + what + " of that frame"); return -1; }
        return tab[i];
    };
    auto single = [&](int b, const char *what) -> int {
        if (index != 0 && index != -1) { set_error(std::string("covariance: ") + what + " index out of range (0)"); return -1; }
        if (b < 0) { set_error(std::string("covariance: the window lacks a requested block: ") + what); return -1; }
        return b;
    };
    int b = -1;
    switch (kind) {
    case TCV_COV_POSE: b = frame(p.frame_pose, "pose"); break;
    case TCV_COV_SPEED_BIAS: b = frame(p.frame_sb, "speed-bias"); break;
    case TCV_COV_EXTRINSIC: b = single(p.proj.empty() ? -1 : p.proj[0].b[2], "extrinsic (no point factors)"); break;
    case TCV_COV_TD: b = single(p.proj.empty() ? -1 : p.proj[0].btd, "td (no para_Td)"); break;
    case TCV_COV_RELO_POSE: b = single(p.relo_block, "relocalisation pose"); break;
    case TCV_COV_LANDMARK: set_error("covariance: landmark (inverse depth) blocks are not supported: camera-side blocks only"); return TCV_ERR_UNSUPPORTED;
    default: set_error("covariance: unknown block kind"); return TCV_ERR_INVALID;
    }
    if (b < 0) return TCV_ERR_INVALID;
    if (blk) *blk = b;
    if (width) *width = block_width(p.blocks[b]);
    return TCV_OK;
}
int check_options(const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks, const char *who) {
    if (!o || !blocks) { set_error(std::string(who) + ": null options or blocks"); return TCV_ERR_INVALID; }
    if (n_blocks < 1 || n_blocks > TCV_COVARIANCE_MAX_BLOCKS) { set_error(std::string(who) + ": n_blocks outside 1 .. TCV_COVARIANCE_MAX_BLOCKS"); return TCV_ERR_INVALID; }
    if (!(o->min_relative_pivot >= 0.0) || !std::isfinite(o->min_relative_pivot)) { set_error(std::string(who) + ": min_relative_pivot must be finite and >= 0"); return TCV_ERR_INVALID; }
    if (o->at_solution != 0 && o->at_solution != 1) { set_error(std::string(who) + ": at_solution must be 0 or 1"); return TCV_ERR_INVALID; }
    return TCV_OK;
}
int check_requests(const tcv_problem &p, const tcv_covariance_block *blocks, int n_blocks) {
    for (int k = 0; k < n_blocks; k++) {
        if (int rc = resolve(p, blocks[k].kind_i, blocks[k].index_i, nullptr, nullptr)) return rc;
        if (int rc = resolve(p, blocks[k].kind_j, blocks[k].index_j, nullptr, nullptr)) return rc;
    }
    return TCV_OK;
}

// Owner lists of S for the plan of window w (tcv_cov.h): a function of the plan's tables alone, rebuilt here from the problem the plan was
// packed from.  `jdoubles`: doubles of the J region.  `lt` (the landmark call only, else null): the plan's landmark slot table
// (tcv_cov.h), the same slots as hslot with their tangent offsets.
int owner_lists(const tcv_batch *b, int w, std::vector<int> &out, int *jdoubles, std::vector<int> *lt = nullptr) {
    const tcv_problem &p = *b->problems[w];
    const Packed &pk = b->packed[w];
    const PlanHdr &H = b->plans[b->wins[w].plan];
    std::vector<int> cam_of(p.blocks.size(), -1), lm_of(p.blocks.size(), -1);
    for (size_t c = 0; c < pk.cam_block.size(); c++) cam_of[pk.cam_block[c]] = (int)c;
    for (size_t l = 0; l < pk.lm_block.size(); l++) lm_of[pk.lm_block[l]] = (int)l;
    auto toff = [&](int blk) { return cam_of[blk] >= 0 ? pk.cam_loff[cam_of[blk]] : -1; };
    struct Pair { int wa = 0, wb = 0, pca = -1, pcb = -1; std::vector<int> items; };
    std::map<std::pair<int, int>, Pair> pairs;
    bool repeated = false;
    // one item of the pair (block A, block B): offsets of the two column blocks in the J region
    auto add = [&](int A, int offA, int B, int offB, int rows, int stride, int sc) {
        int ta = toff(A), tb = toff(B);
        if (ta < 0 || tb < 0) return;
        if (A == B && offA != offB) repeated = true;
        if (ta < tb) { std::swap(ta, tb); std::swap(A, B); std::swap(offA, offB); }
        Pair &q = pairs[{ta, tb}];
        q.wa = block_width(p.blocks[A]); q.wb = block_width(p.blocks[B]);
        const int it[4] = {offA, offB, rows << 16 | stride, sc};
        q.items.insert(q.items.end(), it, it + 4);
    };
    const int L = H.nland, o_proj = COV_J_IMU * H.n_imu, o_line = o_proj + COV_J_PROJ * H.n_proj, o_hll = o_line + COV_J_LINE * H.n_line, o_h = o_hll + 2 * L;
    for (size_t f = 0; f < p.imu.size(); f++) {
        static const int col0[4] = {0, 6, 15, 21};
        for (int x = 0; x < 4; x++) for (int y = 0; y <= x; y++)
            add(p.imu[f].b[x], (int)f * COV_J_IMU + col0[x], p.imu[f].b[y], (int)f * COV_J_IMU + col0[y], 15, 30, -1);
    }
    std::vector<std::vector<int>> lm_fac(L);
    for (size_t k = 0; k < pk.proj_order.size(); k++) {
        const ProjFac &f = p.proj[pk.proj_order[k]];
        const int bl[4] = {f.b[0], f.b[1], f.b[2], f.btd}, col0[4] = {0, 6, 12, 19}, base = o_proj + (int)k * COV_J_PROJ;
        for (int x = 0; x < 4; x++) for (int y = 0; y <= x; y++)
            if (bl[x] >= 0 && bl[y] >= 0) add(bl[x], base + col0[x], bl[y], base + col0[y], 2, 20, -1);
        const int l = lm_of[f.b[3]];
        if (l < 0 || p.blocks[f.b[3]].constant) { set_error("covariance: a constant inverse depth is not supported"); return TCV_ERR_UNSUPPORTED; }
        lm_fac[l].push_back((int)k);
    }
    for (size_t k = 0; k < p.line.size(); k++) add(p.line[k].b, o_line + (int)k * COV_J_LINE, p.line[k].b, o_line + (int)k * COV_J_LINE, 2, 6, -1);
    // landmarks: the slots of h_l (distinct variable blocks in order of first appearance), their owner lists, and the pair items
    std::vector<int> hslot, hitem, lmptr(1, 0), lmfac, lsptr(1, 0), lslot;
    int h_doubles = 0;
    for (int l = 0; l < L; l++) {
        std::vector<int> sblk;
        std::vector<std::vector<int>> sitems;
        for (int k : lm_fac[l]) {
            const ProjFac &f = p.proj[pk.proj_order[k]];
            const int bl[4] = {f.b[0], f.b[1], f.b[2], f.btd}, col0[4] = {0, 6, 12, 19}, base = o_proj + k * COV_J_PROJ;
            for (int x = 0; x < 4; x++) {
                if (bl[x] < 0 || toff(bl[x]) < 0) continue;
                size_t s = std::find(sblk.begin(), sblk.end(), bl[x]) - sblk.begin();
                if (s == sblk.size()) { sblk.push_back(bl[x]); sitems.emplace_back(); }
                sitems[s].push_back(base + col0[x]); sitems[s].push_back(base + 18);
            }
            lmfac.push_back(k);
        }
        lmptr.push_back((int)lmfac.size());
        std::vector<int> soff(sblk.size());
        for (size_t s = 0; s < sblk.size(); s++) {
            soff[s] = o_h + h_doubles; h_doubles += COV_SLOT;
            const int rec[4] = {soff[s], block_width(p.blocks[sblk[s]]), (int)hitem.size() / CT_HITEM, (int)(hitem.size() + sitems[s].size()) / CT_HITEM};
            hslot.insert(hslot.end(), rec, rec + 4);
            hitem.insert(hitem.end(), sitems[s].begin(), sitems[s].end());
        }
        for (size_t x = 0; x < sblk.size(); x++) for (size_t y = 0; y <= x; y++) add(sblk[x], soff[x], sblk[y], soff[y], 1, 0, o_hll + 2 * l);
        if (!lt) continue;
        std::vector<std::pair<int, size_t>> by_row;
        for (size_t x = 0; x < sblk.size(); x++) by_row.push_back({toff(sblk[x]), x});
        std::sort(by_row.begin(), by_row.end());
        for (auto &r : by_row) { const int rec[LT_SLOT] = {r.first, soff[r.second], block_width(p.blocks[sblk[r.second]])}; lslot.insert(lslot.end(), rec, rec + LT_SLOT); }
        lsptr.push_back((int)lslot.size() / LT_SLOT);
    }
    if (lt) { *lt = lsptr; lt->insert(lt->end(), lslot.begin(), lslot.end()); }
    if (repeated) { set_error("covariance: a factor that names one parameter block twice is not supported"); return TCV_ERR_UNSUPPORTED; }
    // the prior: every pair of its variable blocks
    if (H.prior_n > 0 && !p.prior.empty()) {
        const tcv_prior *pr = p.prior[0].prior;
        const std::vector<int> &pb = p.prior[0].b;
        for (size_t x = 0; x < pb.size(); x++) for (size_t y = 0; y < pb.size(); y++) {
            const int ta = toff(pb[x]), tb = toff(pb[y]);
            if (ta < 0 || tb < 0 || ta < tb) continue;
            Pair &q = pairs[{ta, tb}];
            q.wa = block_width(p.blocks[pb[x]]); q.wb = block_width(p.blocks[pb[y]]);
            q.pca = pr->idx[x]; q.pcb = pr->idx[y];
        }
    }
    out.assign(CT_HDR, 0);
    out[CT_NPAIR] = (int)pairs.size(); out[CT_OPAIR] = CT_HDR;
    std::vector<int> items;
    for (auto &kv : pairs) {
        const Pair &q = kv.second;
        const int rec[CT_PAIR] = {kv.first.first, kv.first.second, q.wa, q.wb, (int)items.size() / CT_ITEM, (int)(items.size() + q.items.size()) / CT_ITEM, q.pca, q.pcb};
        out.insert(out.end(), rec, rec + CT_PAIR);
        items.insert(items.end(), q.items.begin(), q.items.end());
    }
    auto put = [&](int slot, const std::vector<int> &v) { out[slot] = (int)out.size(); out.insert(out.end(), v.begin(), v.end()); };
    put(CT_OITEM, items);
    out[CT_NHSLOT] = (int)hslot.size() / CT_HSLOT;
    put(CT_OHSLOT, hslot); put(CT_OHITEM, hitem); put(CT_OLMPTR, lmptr); put(CT_OLMFAC, lmfac);
    out[CT_JPROJ] = o_proj; out[CT_JLINE] = o_line; out[CT_JHLL] = o_hll; out[CT_JDOUBLES] = o_h + h_doubles;
    *jdoubles = o_h + h_doubles;
    return TCV_OK;
}
// first computation of a batch: the owner lists of its distinct plans go up, the work buffers are allocated (returned by tcv_batch_destroy)
int cov_prepare(tcv_batch *b) {
    if (b->cov) return TCV_OK;
    std::unique_ptr<CovState> s(new CovState());
    const int n = b->n, np = (int)b->plans.size();
    for (auto &H : b->plans) {
        if (H.nc > TCV_COVARIANCE_MAX_DIM) { set_error("covariance: more than TCV_COVARIANCE_MAX_DIM camera-side tangent dimensions"); return TCV_ERR_UNSUPPORTED; }
        s->nc_max = std::max(s->nc_max, H.nc);
    }
    std::vector<long long> base(np, -1);
    std::vector<int> ints, one;
    for (int w = 0; w < n; w++) {
        const int pl = b->wins[w].plan;
        if (base[pl] >= 0) continue;
        base[pl] = (long long)ints.size();
        int jd = 0;
        if (int rc = owner_lists(b, w, one, &jd)) return rc;
        ints.insert(ints.end(), one.begin(), one.end());
        const PlanHdr &H = b->plans[pl];
        s->stage_stride = std::max<long long>(s->stage_stride, ((long long)H.n_imu * (225 + IMU_REC) + jd + 1) & ~1LL);
    }
    s->grid = std::min(n, std::max(1, b->n_cu));      // one workgroup per CU (LDS): a persistent grid walks the batch
    const size_t tab_head = sizeof(long long) * (size_t)np, tab_bytes = tab_head + sizeof(int) * std::max<size_t>(1, ints.size());
    const size_t work = sizeof(double) * (size_t)s->grid * ((size_t)s->stage_stride + (size_t)COV_MAX_DIM * COV_MAX_DIM);
    struct Guard { CovState *s; ~Guard() { if (s) { tcv::dev_free(s->d_tab); tcv::dev_free(s->d_work); } } } guard{s.get()};
    hipError_t e = tcv::dev_malloc(&s->d_tab, tab_bytes);
    if (e == hipSuccess) e = tcv::dev_malloc(&s->d_work, work);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (covariance buffers)");
    {
        tcv::StagedTransfer up(tcv::util_stream(), tab_bytes);
        if (!up.host) { set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
        std::memcpy(up.host, base.data(), tab_head);
        if (!ints.empty()) std::memcpy((char *)up.host + tab_head, ints.data(), sizeof(int) * ints.size());
        up.issued();
        e = hipMemcpyAsync(s->d_tab, up.host, tab_bytes, hipMemcpyHostToDevice, up.st);
        const hipError_t ew = up.wait();
        if (e == hipSuccess) e = ew;
        if (e != hipSuccess) return hip_fail(e, "upload of the covariance tables");
    }
    s->d_tab_base = (long long *)s->d_tab; s->d_tab_ints = (int *)((char *)s->d_tab + tab_head);
    s->d_stage = (double *)s->d_work; s->d_y = s->d_stage + (size_t)s->grid * s->stage_stride;
    guard.s = nullptr;
    b->cov = s.release();
    b->cov_free = cov_free;
    return TCV_OK;
}
bool same_requests(const std::vector<tcv_covariance_block> &a, const tcv_covariance_block *blocks, int n) {
    if ((int)a.size() != n) return false;
    for (int k = 0; k < n; k++)
        if (a[k].kind_i != blocks[k].kind_i || a[k].index_i != blocks[k].index_i || a[k].kind_j != blocks[k].kind_j || a[k].index_j != blocks[k].index_j) return false;
    return true;
}
// the request tables of every window (tcv_cov.h RQ_*) for a request list, and the sizes of its blocks
int request_tables(const tcv_batch *b, const tcv_covariance_block *blocks, int n_req, std::vector<int> &rq, std::vector<int> &rows, std::vector<int> &cols) {
    const int n = b->n, stride = cov_rq_stride(n_req);
    rq.assign((size_t)n * stride, 0); rows.assign(n_req, 0); cols.assign(n_req, 0);
    for (int w = 0; w < n; w++) {
        const tcv_problem &p = *b->problems[w];
        const Packed &pk = b->packed[w];
        std::vector<int> cam_of(p.blocks.size(), -1);
        for (size_t c = 0; c < pk.cam_block.size(); c++) cam_of[pk.cam_block[c]] = (int)c;
        int *q = rq.data() + (size_t)w * stride, m = 0;
        std::map<int, int> col_of;      // first tangent index of a block -> its first solved column
        auto column = [&](int blk, int width) -> int {
            const int t = cam_of[blk] >= 0 ? pk.cam_loff[cam_of[blk]] : -1;
            if (t < 0) return -1;
            auto it = col_of.find(t);
            if (it != col_of.end()) return it->second;
            for (int j = 0; j < width; j++) q[RQ_COL + m + j] = t + j;
            col_of[t] = m; m += width;
            return m - width;
        };
        for (int k = 0; k < n_req; k++) {
            int bi = -1, bj = -1, wi = 0, wj = 0;
            if (int rc = resolve(p, blocks[k].kind_i, blocks[k].index_i, &bi, &wi)) return rc;
            if (int rc = resolve(p, blocks[k].kind_j, blocks[k].index_j, &bj, &wj)) return rc;
            if (cam_of[bi] < 0 || cam_of[bj] < 0) { set_error("covariance: a requested block is not on the camera side of the window"); return TCV_ERR_INVALID; }
            if (w > 0 && (wi != rows[k] || wj != cols[k])) { set_error("covariance: a requested block has different sizes in two windows"); return TCV_ERR_INVALID; }
            rows[k] = wi; cols[k] = wj;
            int *r = q + RQ_REQ + 4 * k;
            r[0] = column(bi, wi); r[1] = wi; r[2] = column(bj, wj); r[3] = wj;
        }
        q[RQ_M] = m; q[RQ_NREQ] = n_req;
    }
    return TCV_OK;
}
// a new request list: its tables go up, the result buffers behind them replace the old ones
int cov_requests(tcv_batch *b, CovState *s, const tcv_covariance_block *blocks, int n_req) {
    const int n = b->n;
    std::vector<int> rq, rows, cols;
    if (int rc = request_tables(b, blocks, n_req, rq, rows, cols)) return rc;
    const size_t rq_bytes = (sizeof(int) * rq.size() + 7) & ~(size_t)7, st_bytes = (sizeof(int) * (size_t)n + 7) & ~(size_t)7;
    void *d_res = nullptr;
    hipError_t e = tcv::dev_malloc(&d_res, rq_bytes + st_bytes + sizeof(double) * (size_t)n * n_req * COV_BLOCK_DOUBLES);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (covariance results)");
    {
        tcv::StagedTransfer up(tcv::util_stream(), rq_bytes);
        if (!up.host) { tcv::dev_free(d_res); set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
        std::memcpy(up.host, rq.data(), sizeof(int) * rq.size());
        up.issued();
        e = hipMemcpyAsync(d_res, up.host, rq_bytes, hipMemcpyHostToDevice, up.st);
        const hipError_t ew = up.wait();
        if (e == hipSuccess) e = ew;
        if (e != hipSuccess) { tcv::dev_free(d_res); return hip_fail(e, "upload of the covariance requests"); }
    }
    if (b->pending) if (int rc = tcv_batch_synchronize(b)) { tcv::dev_free(d_res); return rc; }      // a computation in flight still writes the old buffers
    tcv::dev_free(s->d_res);
    s->d_res = d_res;
    s->d_rq = (int *)d_res; s->d_status = (int *)((char *)d_res + rq_bytes); s->d_out = (double *)((char *)d_res + rq_bytes + st_bytes);
    s->req.assign(blocks, blocks + n_req); s->rows = rows; s->cols = cols;
    s->computed = false;
    return TCV_OK;
}
int cov_ready(tcv_batch *b, const char *who) {
    if (!b) { set_error(std::string(who) + ": null batch"); return TCV_ERR_INVALID; }
    if (!b->cov || !((CovState *)b->cov)->computed) { set_error(std::string(who) + ": no covariance has been computed on the batch"); return TCV_ERR_INVALID; }
    if (b->pending) return tcv_batch_synchronize(b);
    return TCV_OK;
}
}  // namespace

extern "C" void tcv_covariance_options_default(tcv_covariance_options *o) {
    if (!o) return;
    o->at_solution = 0;
    o->apply_loss_function = 1;
    o->min_relative_pivot = TCV_COVARIANCE_MIN_RELATIVE_PIVOT;
}
extern "C" int tcv_covariance_pivot_status(double d, double s, double min_relative_pivot) { return tcv::cov_pivot_status(d, s, min_relative_pivot); }

extern "C" int tcv_batch_compute_covariance(tcv_batch *b, const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks, void *hip_stream) {
    if (!b) { set_error("batch_compute_covariance: null batch"); return TCV_ERR_INVALID; }
    if (int rc = check_options(o, blocks, n_blocks, "batch_compute_covariance")) return rc;
    if (o->at_solution && !b->solved) { set_error("batch_compute_covariance: at_solution = 1, but the batch has not been solved"); return TCV_ERR_INVALID; }
    for (int w = 0; w < b->n; w++) if (int rc = check_requests(*b->problems[w], blocks, n_blocks)) return rc;
    if (hip_stream == TCV_STREAM_THREAD) hip_stream = (void *)tcv::util_stream();
    if (int rc = cov_prepare(b)) return rc;
    CovState *s = (CovState *)b->cov;
    if (!same_requests(s->req, blocks, n_blocks)) if (int rc = cov_requests(b, s, blocks, n_blocks)) return rc;
    CovArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->d_win; a.plans = b->d_plans; a.plan_base = b->d_plan_base; a.ipool = b->d_ipool; a.dpool = b->d_dpool;
    a.state = o->at_solution ? b->d_state : nullptr;
    a.tab_base = s->d_tab_base; a.tab = s->d_tab_ints; a.rq = s->d_rq;
    a.stage = s->d_stage; a.ybuf = s->d_y; a.out = s->d_out; a.status = s->d_status;
    a.stage_stride = s->stage_stride;
    a.nwin = b->n; a.state_stride = b->state_stride; a.rq_stride = cov_rq_stride(n_blocks); a.n_req = n_blocks;
    a.apply_loss = o->apply_loss_function ? 1 : 0; a.lds_area = cov_lds_area(b->state_stride, s->nc_max);
    a.min_relative_pivot = o->min_relative_pivot;
    if (int rc = tcv_batch_enter_stream(b, hip_stream)) return rc;
    const int rc = tcv_launch_covariance(&a, s->grid, sizeof(double) * (size_t)cov_lds_doubles(b->state_stride, s->nc_max), hip_stream);
    if (rc != 0) return hip_fail((hipError_t)rc, "covariance kernel launch");
    s->computed = true;
    return TCV_OK;
}
extern "C" int tcv_batch_get_covariance(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = cov_ready(b, "batch_get_covariance")) return rc;
    CovState *s = (CovState *)b->cov;
    const int n_req = (int)s->req.size();
    if (window < 0 || window >= b->n || k < 0 || k >= n_req) { set_error("batch_get_covariance: window or block out of range"); return TCV_ERR_INVALID; }
    const int nel = s->rows[k] * s->cols[k];
    if (!out || cap < nel) { set_error("batch_get_covariance: the output array is missing or too small"); return TCV_ERR_INVALID; }
    double h[COV_BLOCK_DOUBLES];
    if (int rc = tcv::staged_download(h, s->d_out + ((size_t)window * n_req + k) * COV_BLOCK_DOUBLES, sizeof(double) * nel, "download of the covariance")) return rc;
    std::memcpy(out, h, sizeof(double) * nel);
    if (rows) *rows = s->rows[k];
    if (cols) *cols = s->cols[k];
    return TCV_OK;
}
extern "C" int tcv_batch_get_covariance_all(tcv_batch *b, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = cov_ready(b, "batch_get_covariance_all")) return rc;
    CovState *s = (CovState *)b->cov;
    const int n_req = (int)s->req.size(), n = b->n;
    if (k < 0 || k >= n_req) { set_error("batch_get_covariance_all: block out of range"); return TCV_ERR_INVALID; }
    const int nel = s->rows[k] * s->cols[k];
    if (!out || (long long)cap < (long long)nel * n) { set_error("batch_get_covariance_all: the output array is missing or too small"); return TCV_ERR_INVALID; }
    std::vector<double> h((size_t)n * n_req * COV_BLOCK_DOUBLES);
    if (int rc = tcv::staged_download(h.data(), s->d_out, sizeof(double) * h.size(), "download of the covariance")) return rc;
    for (int w = 0; w < n; w++) std::memcpy(out + (size_t)w * nel, h.data() + ((size_t)w * n_req + k) * COV_BLOCK_DOUBLES, sizeof(double) * nel);
    if (rows) *rows = s->rows[k];
    if (cols) *cols = s->cols[k];
    return TCV_OK;
}
extern "C" int tcv_batch_covariance_status(tcv_batch *b, int *out, int n) {
    if (b && (!out || n != b->n)) { set_error("batch_covariance_status: n must be the batch size"); return TCV_ERR_INVALID; }
    if (int rc = cov_ready(b, "batch_covariance_status")) return rc;
    return tcv::staged_download(out, ((CovState *)b->cov)->d_status, sizeof(int) * (size_t)n, "download of the covariance status");
}
// ceres::Covariance for one problem at the caller's current block values: a one-window batch on the calling thread's stream
extern "C" int tcv_problem_compute_covariance(tcv_problem *p, const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks,
                                              double *const *out, int *status) {
    if (!p || !out) { set_error("problem_compute_covariance: null problem or output array"); return TCV_ERR_INVALID; }
    if (int rc = check_options(o, blocks, n_blocks, "problem_compute_covariance")) return rc;
    for (int k = 0; k < n_blocks; k++) if (!out[k]) { set_error("problem_compute_covariance: null output block"); return TCV_ERR_INVALID; }
    if (o->at_solution) { set_error("problem_compute_covariance: at_solution = 1 needs a solved batch (tcv_batch_compute_covariance)"); return TCV_ERR_INVALID; }
    if (int rc = check_requests(*p, blocks, n_blocks)) return rc;
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    int rc = tcv_batch_create(&b, arr, nullptr, nullptr, nullptr, 1);
    if (rc != TCV_OK) return rc;
    rc = tcv_batch_compute_covariance(b, o, blocks, n_blocks, TCV_STREAM_THREAD);
    std::vector<double> h((size_t)n_blocks * COV_BLOCK_DOUBLES);      // the caller's memory is written only when everything came back
    std::vector<int> nel(n_blocks, 0);
    for (int k = 0; k < n_blocks && rc == TCV_OK; k++) {
        int r = 0, c = 0;
        rc = tcv_batch_get_covariance(b, 0, k, h.data() + (size_t)k * COV_BLOCK_DOUBLES, COV_BLOCK_DOUBLES, &r, &c);
        nel[k] = r * c;
    }
    int st = 0;
    if (rc == TCV_OK) rc = tcv_batch_covariance_status(b, &st, 1);
    tcv_batch_destroy(b);
    if (rc != TCV_OK) return rc;
    for (int k = 0; k < n_blocks; k++) std::memcpy(out[k], h.data() + (size_t)k * COV_BLOCK_DOUBLES, sizeof(double) * nel[k]);
    if (status) *status = st;
    return TCV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The landmarks' inverse depths (include/tcv_landmark_covariance.h): phase 7 of the kernel behind the same factorisation.  The cross
// blocks enter the request table as ordinary diagonal requests, so phase 5 solves their columns; the device writes landmarks in plan
// order and whole rows of solved columns, the getters map them to the problem's landmark order and cut the requested blocks out.
namespace {
const char *const LM_WHO = "batch_compute_landmark_covariance";
int lm_check_options(const tcv_covariance_options *o, const tcv_landmark_cross_block *cross, int n_cross, const char *who) {
    if (!o) { set_error(std::string(who) + ": null options"); return TCV_ERR_INVALID; }
    if (n_cross < 0 || n_cross > TCV_LANDMARK_COVARIANCE_MAX_CROSS) { set_error(std::string(who) + ": n_cross outside 0 .. TCV_LANDMARK_COVARIANCE_MAX_CROSS"); return TCV_ERR_INVALID; }
    if (n_cross > 0 && !cross) { set_error(std::string(who) + ": null cross blocks with n_cross > 0"); return TCV_ERR_INVALID; }
    if (!(o->min_relative_pivot >= 0.0) || !std::isfinite(o->min_relative_pivot)) { set_error(std::string(who) + ": min_relative_pivot must be finite and >= 0"); return TCV_ERR_INVALID; }
    if (o->at_solution != 0 && o->at_solution != 1) { set_error(std::string(who) + ": at_solution must be 0 or 1"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n_cross; k++) {
        if (cross[k].kind == TCV_COV_LANDMARK) { set_error(std::string(who) + ": a cross block must be a camera-side block, not a landmark (two landmarks: out of scope)"); return TCV_ERR_INVALID; }
        if (cross[k].kind < TCV_COV_POSE || cross[k].kind > TCV_COV_LANDMARK) { set_error(std::string(who) + ": unknown kind of a cross block"); return TCV_ERR_INVALID; }
    }
    return TCV_OK;
}
int lm_check_cross(const tcv_problem &p, const tcv_landmark_cross_block *cross, int n_cross) {
    for (int k = 0; k < n_cross; k++) if (int rc = resolve(p, cross[k].kind, cross[k].index, nullptr, nullptr)) return rc;
    return TCV_OK;
}
int lm_upload(void *d_dst, const void *src, size_t bytes, const char *what) {
    tcv::StagedTransfer up(tcv::util_stream(), bytes);
    if (!up.host) { set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
    std::memcpy(up.host, src, bytes);
    up.issued();
    hipError_t e = hipMemcpyAsync(d_dst, up.host, bytes, hipMemcpyHostToDevice, up.st);
    const hipError_t ew = up.wait();
    if (e == hipSuccess) e = ew;
    if (e != hipSuccess) return hip_fail(e, what);
    return TCV_OK;
}
// the plan index of every landmark in registration order: the landmarks of a problem are the fourth blocks of its point factors, the
// plan numbers them by first appearance among the factors, the caller by the order the blocks were registered (their block index)
std::vector<int> registration_order(const Packed &pk) {
    std::vector<int> o(pk.lm_block.size());
    for (size_t l = 0; l < o.size(); l++) o[l] = (int)l;
    std::sort(o.begin(), o.end(), [&](int a, int b) { return pk.lm_block[a] < pk.lm_block[b]; });
    return o;
}
// the cross columns are solved by phase 5, one thread per column of at most COV_MAX_DIM
static_assert(TCV_LANDMARK_COVARIANCE_MAX_CROSS * 9 <= COV_MAX_DIM, "the cross blocks' columns must fit the request table");
// first landmark call of a batch: the slot tables of its distinct plans are built and go up, the chunk buffer is allocated (returned by
// tcv_batch_destroy)
int lm_prepare(tcv_batch *b, CovState *s) {
    LmState &m = s->lm;
    if (m.ready) return TCV_OK;
    const int np = (int)b->plans.size();
    std::vector<long long> lt_base(np, -1);
    std::vector<int> lt_ints, lists, lt;
    for (int w = 0; w < b->n; w++) {
        const int pl = b->wins[w].plan;
        if (lt_base[pl] >= 0) continue;
        int jd = 0;
        if (int rc = owner_lists(b, w, lists, &jd, &lt)) return rc;
        lt_base[pl] = (long long)lt_ints.size();
        lt_ints.insert(lt_ints.end(), lt.begin(), lt.end());
    }
    const size_t tab_head = sizeof(long long) * (size_t)np, tab_bytes = tab_head + sizeof(int) * std::max<size_t>(1, lt_ints.size());
    std::vector<char> img(tab_bytes, 0);
    std::memcpy(img.data(), lt_base.data(), tab_head);
    if (!lt_ints.empty()) std::memcpy(img.data() + tab_head, lt_ints.data(), sizeof(int) * lt_ints.size());
    void *d_tab = nullptr, *d_ylm = nullptr;
    hipError_t e = tcv::dev_malloc(&d_tab, tab_bytes);
    if (e == hipSuccess) e = tcv::dev_malloc(&d_ylm, sizeof(double) * (size_t)s->grid * COV_MAX_DIM * COV_LM_CHUNK);
    int rc = e == hipSuccess ? lm_upload(d_tab, img.data(), tab_bytes, "upload of the landmark slot tables") : hip_fail(e, "hipMalloc (landmark covariance buffers)");
    if (rc != TCV_OK) { if (d_tab) tcv::dev_free(d_tab); if (d_ylm) tcv::dev_free(d_ylm); return rc; }
    m.d_tab = d_tab; m.d_ylm = d_ylm;
    m.d_tab_base = (long long *)d_tab; m.d_tab_ints = (int *)((char *)d_tab + tab_head);
    m.plan_of.resize(b->n);
    m.lmax = 0;
    for (int w = 0; w < b->n; w++) { m.plan_of[w] = registration_order(b->packed[w]); m.lmax = std::max(m.lmax, (int)m.plan_of[w].size()); }
    m.ready = true;
    return TCV_OK;
}
bool lm_same_requests(const LmState &m, const tcv_landmark_cross_block *cross, int n) {
    if (!m.have_req || (int)m.req.size() != n) return false;
    for (int k = 0; k < n; k++) if (m.req[k].kind != cross[k].kind || m.req[k].index != cross[k].index) return false;
    return true;
}
// a new cross list: its request tables (the cross blocks as diagonal requests) go up, the result buffers behind them replace the old ones
int lm_requests(tcv_batch *b, CovState *s, const tcv_landmark_cross_block *cross, int n_cross) {
    LmState &m = s->lm;
    const int n = b->n, stride = cov_rq_stride(n_cross);
    std::vector<tcv_covariance_block> diag(n_cross);
    for (int k = 0; k < n_cross; k++) diag[k] = tcv_covariance_block{cross[k].kind, cross[k].index, cross[k].kind, cross[k].index};
    std::vector<int> rq, rows, cols;
    if (int rc = request_tables(b, diag.data(), n_cross, rq, rows, cols)) return rc;
    int mstride = 0;
    for (int w = 0; w < n; w++) mstride = std::max(mstride, rq[(size_t)w * stride + RQ_M]);
    const size_t rq_bytes = (sizeof(int) * rq.size() + 7) & ~(size_t)7, st_bytes = (sizeof(int) * (size_t)n + 7) & ~(size_t)7;
    const size_t out_d = (size_t)n * n_cross * COV_BLOCK_DOUBLES, var_d = (size_t)n * m.lmax, cross_d = (size_t)n * m.lmax * mstride;
    const size_t dbl_bytes = sizeof(double) * std::max<size_t>(1, out_d + var_d + cross_d);
    void *d_res = nullptr;
    hipError_t e = tcv::dev_malloc(&d_res, rq_bytes + st_bytes + dbl_bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (landmark covariance results)");
    int rc = lm_upload(d_res, rq.data(), sizeof(int) * rq.size(), "upload of the landmark covariance requests");
    if (rc == TCV_OK) {      // what no window writes (the tail of a shorter window, columns past its own) reads as zero
        e = hipMemsetAsync((char *)d_res + rq_bytes, 0, st_bytes + dbl_bytes, tcv::util_stream());
        if (e == hipSuccess) e = hipStreamSynchronize(tcv::util_stream());
        if (e != hipSuccess) rc = hip_fail(e, "hipMemset (landmark covariance results)");
    }
    if (rc == TCV_OK && b->pending) rc = tcv_batch_synchronize(b);      // a computation in flight still writes the old buffers
    if (rc != TCV_OK) { tcv::dev_free(d_res); return rc; }
    if (m.d_res) tcv::dev_free(m.d_res);
    m.d_res = d_res;
    m.d_rq = (int *)d_res; m.d_status = (int *)((char *)d_res + rq_bytes);
    m.d_out = (double *)((char *)d_res + rq_bytes + st_bytes); m.d_var = m.d_out + out_d; m.d_cross = m.d_var + var_d;
    m.mstride = mstride; m.rq_stride = stride;
    m.req.assign(cross, cross + n_cross); m.cols = cols; m.rq.swap(rq);
    m.have_req = true; m.computed = false;
    return TCV_OK;
}
int lm_computed(tcv_batch *b, const char *who) {
    if (!b) { set_error(std::string(who) + ": null batch"); return TCV_ERR_INVALID; }
    if (!b->cov || !((CovState *)b->cov)->lm.computed) { set_error(std::string(who) + ": no landmark covariance has been computed on the batch"); return TCV_ERR_INVALID; }
    if (b->pending) return tcv_batch_synchronize(b);
    return TCV_OK;
}
}  // namespace

extern "C" int tcv_batch_compute_landmark_covariance(tcv_batch *b, const tcv_covariance_options *o, const tcv_landmark_cross_block *cross, int n_cross,
                                                     void *hip_stream) {
    if (!b) { set_error(std::string(LM_WHO) + ": null batch"); return TCV_ERR_INVALID; }
    if (int rc = lm_check_options(o, cross, n_cross, LM_WHO)) return rc;
    if (o->at_solution && !b->solved) { set_error(std::string(LM_WHO) + ": at_solution = 1, but the batch has not been solved"); return TCV_ERR_INVALID; }
    for (int w = 0; w < b->n; w++) if (int rc = lm_check_cross(*b->problems[w], cross, n_cross)) return rc;
    if (hip_stream == TCV_STREAM_THREAD) hip_stream = (void *)tcv::util_stream();
    if (int rc = cov_prepare(b)) return rc;
    CovState *s = (CovState *)b->cov;
    if (int rc = lm_prepare(b, s)) return rc;
    LmState &m = s->lm;
    if (!lm_same_requests(m, cross, n_cross)) if (int rc = lm_requests(b, s, cross, n_cross)) return rc;
    CovArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->d_win; a.plans = b->d_plans; a.plan_base = b->d_plan_base; a.ipool = b->d_ipool; a.dpool = b->d_dpool;
    a.state = o->at_solution ? b->d_state : nullptr;
    a.tab_base = s->d_tab_base; a.tab = s->d_tab_ints; a.rq = m.d_rq;
    a.stage = s->d_stage; a.ybuf = s->d_y; a.out = m.d_out; a.status = m.d_status;
    a.stage_stride = s->stage_stride;
    a.nwin = b->n; a.state_stride = b->state_stride; a.rq_stride = m.rq_stride; a.n_req = n_cross;
    a.apply_loss = o->apply_loss_function ? 1 : 0; a.lds_area = cov_lds_area(b->state_stride, s->nc_max);
    a.min_relative_pivot = o->min_relative_pivot;
    a.ltab_base = m.d_tab_base; a.ltab = m.d_tab_ints; a.ylm = (double *)m.d_ylm;
    a.lm_var = m.d_var; a.lm_cross = m.d_cross; a.lm_lmax = m.lmax; a.lm_mstride = m.mstride;
    if (int rc = tcv_batch_enter_stream(b, hip_stream)) return rc;
    const int rc = tcv_launch_landmark_covariance(&a, s->grid, sizeof(double) * (size_t)cov_lds_doubles(b->state_stride, s->nc_max), hip_stream);
    if (rc != 0) return hip_fail((hipError_t)rc, "landmark covariance kernel launch");
    m.computed = true;
    return TCV_OK;
}
extern "C" int tcv_batch_landmark_covariance_dims(tcv_batch *b, int window, int *n_landmarks) {
    if (!b || !n_landmarks) { set_error("batch_landmark_covariance_dims: null batch or output"); return TCV_ERR_INVALID; }
    if (window < 0 || window >= b->n) { set_error("batch_landmark_covariance_dims: window out of range"); return TCV_ERR_INVALID; }
    *n_landmarks = (int)b->packed[window].lm_block.size();
    return TCV_OK;
}
extern "C" int tcv_batch_get_landmark_variances(tcv_batch *b, int window, double *out, int cap, int *n) {
    if (int rc = lm_computed(b, "batch_get_landmark_variances")) return rc;
    const LmState &m = ((CovState *)b->cov)->lm;
    if (window < 0 || window >= b->n) { set_error("batch_get_landmark_variances: window out of range"); return TCV_ERR_INVALID; }
    const std::vector<int> &po = m.plan_of[window];
    const int L = (int)po.size();
    if (!out || cap < L) { set_error("batch_get_landmark_variances: the output array is missing or too small"); return TCV_ERR_INVALID; }
    std::vector<double> h(L);
    if (L > 0) if (int rc = tcv::staged_download(h.data(), m.d_var + (size_t)window * m.lmax, sizeof(double) * L, "download of the landmark variances")) return rc;
    for (int l = 0; l < L; l++) out[l] = h[po[l]];
    if (n) *n = L;
    return TCV_OK;
}
extern "C" int tcv_batch_get_landmark_variances_all(tcv_batch *b, double *out, int cap, int *stride) {
    if (int rc = lm_computed(b, "batch_get_landmark_variances_all")) return rc;
    const LmState &m = ((CovState *)b->cov)->lm;
    const size_t nel = (size_t)b->n * m.lmax;
    if (!out || (long long)cap < (long long)nel) { set_error("batch_get_landmark_variances_all: the output array is missing or too small"); return TCV_ERR_INVALID; }
    std::vector<double> h(nel);
    if (nel > 0) if (int rc = tcv::staged_download(h.data(), m.d_var, sizeof(double) * nel, "download of the landmark variances")) return rc;
    for (int w = 0; w < b->n; w++) {
        const std::vector<int> &po = m.plan_of[w];
        double *o = out + (size_t)w * m.lmax;
        for (int l = 0; l < m.lmax; l++) o[l] = l < (int)po.size() ? h[(size_t)w * m.lmax + po[l]] : 0.0;
    }
    if (stride) *stride = m.lmax;
    return TCV_OK;
}
extern "C" int tcv_batch_get_landmark_cross(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = lm_computed(b, "batch_get_landmark_cross")) return rc;
    const LmState &m = ((CovState *)b->cov)->lm;
    if (window < 0 || window >= b->n || k < 0 || k >= (int)m.req.size()) { set_error("batch_get_landmark_cross: window or cross block out of range"); return TCV_ERR_INVALID; }
    const std::vector<int> &po = m.plan_of[window];
    const int L = (int)po.size(), wk = m.cols[k];
    if (!out || (long long)cap < (long long)L * wk) { set_error("batch_get_landmark_cross: the output array is missing or too small"); return TCV_ERR_INVALID; }
    const int c0 = m.rq[(size_t)window * m.rq_stride + RQ_REQ + 4 * k];      // first solved column of the block; -1: constant in this window
    std::vector<double> h((size_t)L * m.mstride);
    if (c0 >= 0 && !h.empty())
        if (int rc = tcv::staged_download(h.data(), m.d_cross + (size_t)window * m.lmax * m.mstride, sizeof(double) * h.size(), "download of the landmark cross covariance")) return rc;
    for (int l = 0; l < L; l++) for (int j = 0; j < wk; j++) out[(size_t)l * wk + j] = c0 >= 0 ? h[(size_t)po[l] * m.mstride + c0 + j] : 0.0;
    if (rows) *rows = L;
    if (cols) *cols = wk;
    return TCV_OK;
}
extern "C" int tcv_batch_landmark_covariance_status(tcv_batch *b, int *out, int n) {
    if (b && (!out || n != b->n)) { set_error("batch_landmark_covariance_status: n must be the batch size"); return TCV_ERR_INVALID; }
    if (int rc = lm_computed(b, "batch_landmark_covariance_status")) return rc;
    return tcv::staged_download(out, ((CovState *)b->cov)->lm.d_status, sizeof(int) * (size_t)n, "download of the landmark covariance status");
}
// one problem at the caller's current block values: a one-window batch on the calling thread's stream; the landmarks by address
extern "C" int tcv_problem_compute_landmark_covariance(tcv_problem *p, const tcv_covariance_options *o, double *const *inv_depth_addresses, int n,
                                                       const tcv_landmark_cross_block *cross, int n_cross, double *variances, double *const *cross_out,
                                                       int *status) {
    const char *who = "problem_compute_landmark_covariance";
    if (!p || !inv_depth_addresses || !variances) { set_error(std::string(who) + ": null problem, address list or variance array"); return TCV_ERR_INVALID; }
    if (n < 1) { set_error(std::string(who) + ": n must be at least 1"); return TCV_ERR_INVALID; }
    if (int rc = lm_check_options(o, cross, n_cross, who)) return rc;
    if (n_cross > 0 && !cross_out) { set_error(std::string(who) + ": null cross output array with n_cross > 0"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n_cross; k++) if (!cross_out[k]) { set_error(std::string(who) + ": null cross output block"); return TCV_ERR_INVALID; }
    if (o->at_solution) { set_error(std::string(who) + ": at_solution = 1 needs a solved batch (tcv_batch_compute_landmark_covariance)"); return TCV_ERR_INVALID; }
    if (int rc = lm_check_cross(*p, cross, n_cross)) return rc;
    // the problem's landmarks in registration order: the fourth blocks of its point factors, by block index
    std::vector<int> rank(p->blocks.size(), -1);
    for (auto &f : p->proj) rank[f.b[3]] = 0;
    int L = 0;
    for (size_t k = 0; k < rank.size(); k++) if (rank[k] == 0) rank[k] = L++;
    std::vector<int> which(n);
    for (int i = 0; i < n; i++) {
        const int blk = p->index.find(inv_depth_addresses[i]);
        if (blk < 0 || rank[blk] < 0) { set_error(std::string(who) + ": an address is not an inverse-depth block of the problem (the fourth block of a point factor)"); return TCV_ERR_INVALID; }
        which[i] = rank[blk];
    }
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    int rc = tcv_batch_create(&b, arr, nullptr, nullptr, nullptr, 1);
    if (rc != TCV_OK) return rc;
    rc = tcv_batch_compute_landmark_covariance(b, o, cross, n_cross, TCV_STREAM_THREAD);
    std::vector<double> var((size_t)std::max(1, L));      // the caller's memory is written only when everything came back
    std::vector<std::vector<double>> cr(n_cross);
    std::vector<int> wk(n_cross, 0);
    int nl = 0, st = 0;
    if (rc == TCV_OK) rc = tcv_batch_get_landmark_variances(b, 0, var.data(), (int)var.size(), &nl);
    if (rc == TCV_OK && nl != L) { set_error(std::string(who) + ": the batch holds another number of landmarks than the problem"); rc = TCV_ERR_INVALID; }
    for (int k = 0; k < n_cross && rc == TCV_OK; k++) {
        int r = 0;
        cr[k].assign((size_t)std::max(1, L) * 9, 0.0);
        rc = tcv_batch_get_landmark_cross(b, 0, k, cr[k].data(), (int)cr[k].size(), &r, &wk[k]);
    }
    if (rc == TCV_OK) rc = tcv_batch_landmark_covariance_status(b, &st, 1);
    tcv_batch_destroy(b);
    if (rc != TCV_OK) return rc;
    for (int i = 0; i < n; i++) variances[i] = var[which[i]];
    for (int k = 0; k < n_cross; k++) for (int i = 0; i < n; i++) std::memcpy(cross_out[k] + (size_t)i * wk[k], cr[k].data() + (size_t)which[i] * wk[k], sizeof(double) * wk[k]);
    if (status) *status = st;
    return TCV_OK;
}
