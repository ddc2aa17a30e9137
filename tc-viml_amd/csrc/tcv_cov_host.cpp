// Host half of the batched marginal covariance (include/tcv_covariance.h, include/tcv_landmark_covariance.h; the kernel: tcv_cov.hip):
// the buffers of a batch and the C-ABI of both calls.  The plain call and the landmark call share the owner lists, the work buffers, one
// result-buffer routine and one launch routine; each keeps a result buffer of its own, and the landmark call adds its slot tables and its
// chunk buffer at its first use.  The tables themselves are built by tcv_cov_tables.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/tcv_covariance.h"
#include "../../include/tcv_landmark_covariance.h"
#include "tcv_cov.h"
#include "tcv_host.h"

using namespace tcv;

extern "C" int tcv_launch_covariance(const tcv::CovArgs *args, int grid, size_t lds_bytes, void *stream, bool landmarks);
namespace {
// the cross columns are solved by phase 5, one thread per column of at most COV_MAX_DIM
static_assert(TCV_LANDMARK_COVARIANCE_MAX_CROSS * 9 <= COV_MAX_DIM, "the cross blocks' columns must fit the request table");
static_assert((int)COV_MAX_DIM == TCV_COVARIANCE_MAX_DIM, "the kernel's limit is the one the header promises");
// the results of one of the two calls: one allocation [request tables | status | doubles] for its last request list
struct ResultBuf {
    void *d = nullptr;
    int *rq = nullptr, *status = nullptr;
    double *out = nullptr;                      // per window n_req x COV_BLOCK_DOUBLES; whatever else the call keeps lies behind them
    std::vector<tcv_covariance_block> req;      // the last request list (the landmark call: its cross blocks as diagonal requests)
    std::vector<int> rows, cols;                // sizes of its blocks
    bool have_req = false, computed = false;
};
// the landmark call's half of a batch's covariance state (made at the first tcv_batch_compute_landmark_covariance)
struct LmState {
    PlanTable tab;              // the slot table of every plan
    void *d_ylm = nullptr;      // y_l of a chunk, per workgroup
    ResultBuf res;              // doubles: [diagonal blocks of the cross requests | variances | cross rows]
    double *d_var = nullptr, *d_cross = nullptr;
    int lmax = 0, mstride = 0;
    bool ready = false;
    std::vector<int> rq;                            // host copy of the request tables (first solved column of every block per window)
    std::vector<std::vector<int>> plan_of;          // per window: plan index of the l-th landmark in registration order
};
struct CovState : tcv::SideState {
    PlanTable tab;              // the owner lists of every plan
    void *d_work = nullptr;     // [staging | y] per workgroup
    ResultBuf res;              // doubles: the blocks
    double *d_stage = nullptr, *d_y = nullptr;
    long long stage_stride = 0;
    int grid = 0, nc_max = 0;
    LmState lm;
    ~CovState() override {
        tcv::dev_free(tab.d); tcv::dev_free(d_work); tcv::dev_free(res.d);
        tcv::dev_free(lm.tab.d); tcv::dev_free(lm.d_ylm); tcv::dev_free(lm.res.d);
    }
};
CovState *cov_of(const tcv_batch *b) { return static_cast<CovState *>(b->cov.get()); }
// what both calls ask of their options
int check_options(const tcv_covariance_options *o, const char *who) {
    if (!(o->min_relative_pivot >= 0.0) || !std::isfinite(o->min_relative_pivot)) { set_error(std::string(who) + ": min_relative_pivot must be finite and >= 0"); return TCV_ERR_INVALID; }
    if (o->at_solution != 0 && o->at_solution != 1) { set_error(std::string(who) + ": at_solution must be 0 or 1"); return TCV_ERR_INVALID; }
    return TCV_OK;
}
int check_plain(const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks, const char *who) {
    if (!o || !blocks) { set_error(std::string(who) + ": null options or blocks"); return TCV_ERR_INVALID; }
    if (n_blocks < 1 || n_blocks > TCV_COVARIANCE_MAX_BLOCKS) { set_error(std::string(who) + ": n_blocks outside 1 .. TCV_COVARIANCE_MAX_BLOCKS"); return TCV_ERR_INVALID; }
    return check_options(o, who);
}
int check_landmark(const tcv_covariance_options *o, const tcv_landmark_cross_block *cross, int n_cross, const char *who) {
    if (!o) { set_error(std::string(who) + ": null options"); return TCV_ERR_INVALID; }
    if (n_cross < 0 || n_cross > TCV_LANDMARK_COVARIANCE_MAX_CROSS) { set_error(std::string(who) + ": n_cross outside 0 .. TCV_LANDMARK_COVARIANCE_MAX_CROSS"); return TCV_ERR_INVALID; }
    if (n_cross > 0 && !cross) { set_error(std::string(who) + ": null cross blocks with n_cross > 0"); return TCV_ERR_INVALID; }
    if (int rc = check_options(o, who)) return rc;
    for (int k = 0; k < n_cross; k++) {
        if (cross[k].kind == TCV_COV_LANDMARK) { set_error(std::string(who) + ": a cross block must be a camera-side block, not a landmark (two landmarks: out of scope)"); return TCV_ERR_INVALID; }
        if (cross[k].kind < TCV_COV_POSE || cross[k].kind > TCV_COV_LANDMARK) { set_error(std::string(who) + ": unknown kind of a cross block"); return TCV_ERR_INVALID; }
    }
    return TCV_OK;
}
// every block of a request list exists in the problem
int check_requests(const tcv_problem &p, const tcv_covariance_block *blocks, int n_blocks) {
    for (int k = 0; k < n_blocks; k++) {
        if (int rc = cov_resolve(p, blocks[k].kind_i, blocks[k].index_i, nullptr, nullptr)) return rc;
        if (int rc = cov_resolve(p, blocks[k].kind_j, blocks[k].index_j, nullptr, nullptr)) return rc;
    }
    return TCV_OK;
}
// a cross list as the request list the kernel sees: every cross block as a diagonal request, so that phase 5 solves its columns
std::vector<tcv_covariance_block> diagonal_requests(const tcv_landmark_cross_block *cross, int n_cross) {
    std::vector<tcv_covariance_block> diag(n_cross);
    for (int k = 0; k < n_cross; k++) diag[k] = tcv_covariance_block{cross[k].kind, cross[k].index, cross[k].kind, cross[k].index};
    return diag;
}
// first computation of a batch: the owner lists of its distinct plans go up, the work buffers are allocated (returned by tcv_batch_destroy)
int cov_prepare(tcv_batch *b) {
    if (b->cov) return TCV_OK;
    std::unique_ptr<CovState> s(new CovState());
    for (auto &H : b->in.plans) {
        if (H.nc > TCV_COVARIANCE_MAX_DIM) { set_error("covariance: more than TCV_COVARIANCE_MAX_DIM camera-side tangent dimensions"); return TCV_ERR_UNSUPPORTED; }
        s->nc_max = std::max(s->nc_max, H.nc);
    }
    auto entry = [&](int w, std::vector<int> &out) -> int {
        const PlanHdr &H = b->in.plans[b->in.wins[w].plan];
        int jd = 0;
        if (int rc = cov_owner_lists(*b->in.problems[w], b->in.packed[w], H, out, &jd)) return rc;
        s->stage_stride = std::max<long long>(s->stage_stride, ((long long)H.n_imu * (225 + IMU_REC) + jd + 1) & ~1LL);
        return TCV_OK;
    };
    if (int rc = plan_table_create(b, entry, "hipMalloc (covariance buffers)", "upload of the covariance tables", &s->tab)) return rc;
    s->grid = std::min(b->in.n, std::max(1, b->shape.n_cu));      // one workgroup per CU (LDS): a persistent grid walks the batch
    const size_t work = sizeof(double) * (size_t)s->grid * ((size_t)s->stage_stride + (size_t)COV_MAX_DIM * COV_MAX_DIM);
    if (hipError_t e = tcv::dev_malloc(&s->d_work, work)) { tcv::dev_free(s->tab.d); return hip_fail(e, "hipMalloc (covariance buffers)"); }
    s->d_stage = (double *)s->d_work; s->d_y = s->d_stage + (size_t)s->grid * s->stage_stride;
    b->cov = std::move(s);
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
// first landmark call of a batch, behind cov_prepare: the slot tables of its distinct plans are built and go up, the chunk buffer is
// allocated (returned by tcv_batch_destroy)
int lm_prepare(tcv_batch *b, CovState *s) {
    LmState &m = s->lm;
    if (m.ready) return TCV_OK;
    auto entry = [&](int w, std::vector<int> &out) -> int {
        const tcv_problem &p = *b->in.problems[w];
        out = cov_slot_table(p, b->in.packed[w], cov_landmark_slots(p, b->in.packed[w], b->in.plans[b->in.wins[w].plan]));
        return TCV_OK;
    };
    PlanTable tab;
    if (int rc = plan_table_create(b, entry, "hipMalloc (landmark covariance buffers)", "upload of the landmark slot tables", &tab)) return rc;
    void *d_ylm = nullptr;
    if (hipError_t e = tcv::dev_malloc(&d_ylm, sizeof(double) * (size_t)s->grid * COV_MAX_DIM * COV_LM_CHUNK)) { tcv::dev_free(tab.d); return hip_fail(e, "hipMalloc (landmark covariance buffers)"); }
    m.tab = tab; m.d_ylm = d_ylm;
    m.plan_of.resize(b->in.n);
    m.lmax = 0;
    for (int w = 0; w < b->in.n; w++) { m.plan_of[w] = registration_order(b->in.packed[w]); m.lmax = std::max(m.lmax, (int)m.plan_of[w].size()); }
    m.ready = true;
    return TCV_OK;
}
bool same_requests(const ResultBuf &r, const tcv_covariance_block *blocks, int n) {
    if (!r.have_req || (int)r.req.size() != n) return false;
    for (int k = 0; k < n; k++)
        if (r.req[k].kind_i != blocks[k].kind_i || r.req[k].index_i != blocks[k].index_i || r.req[k].kind_j != blocks[k].kind_j || r.req[k].index_j != blocks[k].index_j) return false;
    return true;
}
// a new result buffer [rq | status | `doubles` doubles] replaces the old one: the request tables go up; `zero`: status and doubles are cleared
int result_replace(tcv_batch *b, ResultBuf &r, const std::vector<int> &rq, size_t doubles, bool zero, const std::string &what) {
    const size_t rq_bytes = (sizeof(int) * rq.size() + 7) & ~(size_t)7, st_bytes = (sizeof(int) * (size_t)b->in.n + 7) & ~(size_t)7, tail = st_bytes + sizeof(double) * doubles;
    void *d = nullptr;
    hipError_t e = tcv::dev_malloc(&d, rq_bytes + tail);
    if (e != hipSuccess) return hip_fail(e, ("hipMalloc (" + what + " results)").c_str());
    int rc = tcv::staged_upload(d, rq.data(), sizeof(int) * rq.size(), ("upload of the " + what + " requests").c_str());
    if (rc == TCV_OK && zero) {
        e = hipMemsetAsync((char *)d + rq_bytes, 0, tail, tcv::util_stream());
        if (e == hipSuccess) e = hipStreamSynchronize(tcv::util_stream());
        if (e != hipSuccess) rc = hip_fail(e, ("hipMemset (" + what + " results)").c_str());
    }
    if (rc == TCV_OK) rc = b->settle();      // a computation in flight still writes the old buffers
    if (rc != TCV_OK) { tcv::dev_free(d); return rc; }
    tcv::dev_free(r.d);
    r.d = d; r.rq = (int *)d; r.status = (int *)((char *)d + rq_bytes); r.out = (double *)((char *)d + rq_bytes + st_bytes);
    r.computed = false;
    return TCV_OK;
}
// a new request list of either call: its tables and the result buffer behind them.  The landmark call keeps the variances and the cross
// rows behind the blocks, and clears everything: what no window writes (the tail of a shorter window, columns past its own) reads as zero
int new_requests(tcv_batch *b, CovState *s, bool landmarks, const tcv_covariance_block *blocks, int n_req) {
    LmState &m = s->lm;
    ResultBuf &r = landmarks ? m.res : s->res;
    const size_t n = b->in.n, stride = cov_rq_stride(n_req);
    std::vector<int> rq, rows, cols;
    if (int rc = cov_request_tables(b, blocks, n_req, rq, rows, cols)) return rc;
    int mstride = 0;
    for (size_t w = 0; w < n; w++) mstride = std::max(mstride, rq[w * stride + RQ_M]);
    const size_t out_d = n * n_req * COV_BLOCK_DOUBLES, var_d = landmarks ? n * m.lmax : 0, cross_d = var_d * mstride;
    if (int rc = result_replace(b, r, rq, std::max<size_t>(1, out_d + var_d + cross_d), landmarks, landmarks ? "landmark covariance" : "covariance")) return rc;
    r.req.assign(blocks, blocks + n_req); r.rows = rows; r.cols = cols;
    r.have_req = true;
    if (landmarks) { m.d_var = r.out + out_d; m.d_cross = m.d_var + var_d; m.mstride = mstride; m.rq.swap(rq); }
    return TCV_OK;
}
// either call behind its own argument checks: prepare, tables, launch
int compute(tcv_batch *b, const tcv_covariance_options *o, bool landmarks, const tcv_covariance_block *blocks, int n_req, void *hip_stream, const char *who) {
    if (o->at_solution && !b->last.solved) { set_error(std::string(who) + ": at_solution = 1, but the batch has not been solved"); return TCV_ERR_INVALID; }
    for (int w = 0; w < b->in.n; w++) if (int rc = check_requests(*b->in.problems[w], blocks, n_req)) return rc;
    hip_stream = (void *)tcv::resolve_stream(hip_stream);
    if (int rc = cov_prepare(b)) return rc;
    CovState *s = cov_of(b);
    if (landmarks) if (int rc = lm_prepare(b, s)) return rc;
    const LmState &m = s->lm;
    ResultBuf &r = landmarks ? s->lm.res : s->res;
    if (!same_requests(r, blocks, n_req)) if (int rc = new_requests(b, s, landmarks, blocks, n_req)) return rc;
    CovArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->mem.d_win; a.plans = b->mem.d_plans; a.plan_base = b->mem.d_plan_base; a.ipool = b->mem.d_ipool; a.dpool = b->mem.d_dpool;
    a.state = o->at_solution ? b->mem.d_state : nullptr;
    a.tab_base = s->tab.base; a.tab = s->tab.ints; a.rq = r.rq;
    a.stage = s->d_stage; a.ybuf = s->d_y; a.out = r.out; a.status = r.status;
    a.stage_stride = s->stage_stride;
    a.nwin = b->in.n; a.state_stride = b->in.state_stride; a.rq_stride = cov_rq_stride(n_req); a.n_req = n_req;
    a.apply_loss = o->apply_loss_function ? 1 : 0; a.lds_area = cov_lds_area(b->in.state_stride, s->nc_max);
    a.min_relative_pivot = o->min_relative_pivot;
    if (landmarks) {
        a.ltab_base = m.tab.base; a.ltab = m.tab.ints; a.ylm = (double *)m.d_ylm;
        a.lm_var = m.d_var; a.lm_cross = m.d_cross; a.lm_lmax = m.lmax; a.lm_mstride = m.mstride;
    }
    if (int rc = b->flight.enter((hipStream_t)hip_stream)) return rc;
    const int rc = tcv_launch_covariance(&a, s->grid, sizeof(double) * (size_t)cov_lds_doubles(b->in.state_stride, s->nc_max), hip_stream, landmarks);
    if (rc != 0) return hip_fail((hipError_t)rc, landmarks ? "landmark covariance kernel launch" : "covariance kernel launch");
    r.computed = true;
    return TCV_OK;
}
// the getters' gate: the call has been made, and its results are complete
int computed(tcv_batch *b, bool landmarks, const char *who) {
    if (!b) { set_error(std::string(who) + ": null batch"); return TCV_ERR_INVALID; }
    const CovState *s = cov_of(b);
    if (!s || !(landmarks ? s->lm.res : s->res).computed) {
        set_error(std::string(who) + (landmarks ? ": no landmark covariance has been computed on the batch" : ": no covariance has been computed on the batch"));
        return TCV_ERR_INVALID;
    }
    return b->settle();
}
// one problem at the caller's current block values: a one-window batch on the calling thread's stream, destroyed on every path
template <class Body> int one_window_batch(tcv_problem *p, Body &&body) {
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    int rc = tcv_batch_create(&b, arr, nullptr, nullptr, nullptr, 1);
    if (rc != TCV_OK) return rc;
    rc = body(b);
    tcv_batch_destroy(b);
    return rc;
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
    if (int rc = check_plain(o, blocks, n_blocks, "batch_compute_covariance")) return rc;
    return compute(b, o, false, blocks, n_blocks, hip_stream, "batch_compute_covariance");
}
extern "C" int tcv_batch_get_covariance(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = computed(b, false, "batch_get_covariance")) return rc;
    const ResultBuf &r = cov_of(b)->res;
    const int n_req = (int)r.req.size();
    if (window < 0 || window >= b->in.n || k < 0 || k >= n_req) { set_error("batch_get_covariance: window or block out of range"); return TCV_ERR_INVALID; }
    const int nel = r.rows[k] * r.cols[k];
    if (!out || cap < nel) { set_error("batch_get_covariance: the output array is missing or too small"); return TCV_ERR_INVALID; }
    double h[COV_BLOCK_DOUBLES];
    if (int rc = tcv::staged_download(h, r.out + ((size_t)window * n_req + k) * COV_BLOCK_DOUBLES, sizeof(double) * nel, "download of the covariance")) return rc;
    std::memcpy(out, h, sizeof(double) * nel);
    if (rows) *rows = r.rows[k];
    if (cols) *cols = r.cols[k];
    return TCV_OK;
}
extern "C" int tcv_batch_get_covariance_all(tcv_batch *b, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = computed(b, false, "batch_get_covariance_all")) return rc;
    const ResultBuf &r = cov_of(b)->res;
    const int n_req = (int)r.req.size(), n = b->in.n;
    if (k < 0 || k >= n_req) { set_error("batch_get_covariance_all: block out of range"); return TCV_ERR_INVALID; }
    const int nel = r.rows[k] * r.cols[k];
    if (!out || (long long)cap < (long long)nel * n) { set_error("batch_get_covariance_all: the output array is missing or too small"); return TCV_ERR_INVALID; }
    std::vector<double> h((size_t)n * n_req * COV_BLOCK_DOUBLES);
    if (int rc = tcv::staged_download(h.data(), r.out, sizeof(double) * h.size(), "download of the covariance")) return rc;
    for (int w = 0; w < n; w++) std::memcpy(out + (size_t)w * nel, h.data() + ((size_t)w * n_req + k) * COV_BLOCK_DOUBLES, sizeof(double) * nel);
    if (rows) *rows = r.rows[k];
    if (cols) *cols = r.cols[k];
    return TCV_OK;
}
extern "C" int tcv_batch_covariance_status(tcv_batch *b, int *out, int n) {
    if (b && (!out || n != b->in.n)) { set_error("batch_covariance_status: n must be the batch size"); return TCV_ERR_INVALID; }
    if (int rc = computed(b, false, "batch_covariance_status")) return rc;
    return tcv::staged_download(out, cov_of(b)->res.status, sizeof(int) * (size_t)n, "download of the covariance status");
}
// ceres::Covariance for one problem at the caller's current block values
extern "C" int tcv_problem_compute_covariance(tcv_problem *p, const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks,
                                              double *const *out, int *status) {
    if (!p || !out) { set_error("problem_compute_covariance: null problem or output array"); return TCV_ERR_INVALID; }
    if (int rc = check_plain(o, blocks, n_blocks, "problem_compute_covariance")) return rc;
    for (int k = 0; k < n_blocks; k++) if (!out[k]) { set_error("problem_compute_covariance: null output block"); return TCV_ERR_INVALID; }
    if (o->at_solution) { set_error("problem_compute_covariance: at_solution = 1 needs a solved batch (tcv_batch_compute_covariance)"); return TCV_ERR_INVALID; }
    if (int rc = check_requests(*p, blocks, n_blocks)) return rc;
    std::vector<double> h((size_t)n_blocks * COV_BLOCK_DOUBLES);      // the caller's memory is written only when everything came back
    std::vector<int> nel(n_blocks, 0);
    int st = 0;
    const int rc = one_window_batch(p, [&](tcv_batch *b) {
        int rc = tcv_batch_compute_covariance(b, o, blocks, n_blocks, TCV_STREAM_THREAD);
        for (int k = 0; k < n_blocks && rc == TCV_OK; k++) {
            int r = 0, c = 0;
            rc = tcv_batch_get_covariance(b, 0, k, h.data() + (size_t)k * COV_BLOCK_DOUBLES, COV_BLOCK_DOUBLES, &r, &c);
            nel[k] = r * c;
        }
        return rc == TCV_OK ? tcv_batch_covariance_status(b, &st, 1) : rc;
    });
    if (rc != TCV_OK) return rc;
    for (int k = 0; k < n_blocks; k++) std::memcpy(out[k], h.data() + (size_t)k * COV_BLOCK_DOUBLES, sizeof(double) * nel[k]);
    if (status) *status = st;
    return TCV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The landmarks' inverse depths (include/tcv_landmark_covariance.h): phase 7 of the kernel behind the same factorisation.  The cross
// blocks enter the request table as ordinary diagonal requests, so phase 5 solves their columns; the device writes landmarks in plan
// order and whole rows of solved columns, the getters map them to the problem's landmark order and cut the requested blocks out.
extern "C" int tcv_batch_compute_landmark_covariance(tcv_batch *b, const tcv_covariance_options *o, const tcv_landmark_cross_block *cross, int n_cross,
                                                     void *hip_stream) {
    const char *who = "batch_compute_landmark_covariance";
    if (!b) { set_error(std::string(who) + ": null batch"); return TCV_ERR_INVALID; }
    if (int rc = check_landmark(o, cross, n_cross, who)) return rc;
    return compute(b, o, true, diagonal_requests(cross, n_cross).data(), n_cross, hip_stream, who);
}
extern "C" int tcv_batch_landmark_covariance_dims(tcv_batch *b, int window, int *n_landmarks) {
    if (!b || !n_landmarks) { set_error("batch_landmark_covariance_dims: null batch or output"); return TCV_ERR_INVALID; }
    if (window < 0 || window >= b->in.n) { set_error("batch_landmark_covariance_dims: window out of range"); return TCV_ERR_INVALID; }
    *n_landmarks = (int)b->in.packed[window].lm_block.size();
    return TCV_OK;
}
extern "C" int tcv_batch_get_landmark_variances(tcv_batch *b, int window, double *out, int cap, int *n) {
    if (int rc = computed(b, true, "batch_get_landmark_variances")) return rc;
    const LmState &m = cov_of(b)->lm;
    if (window < 0 || window >= b->in.n) { set_error("batch_get_landmark_variances: window out of range"); return TCV_ERR_INVALID; }
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
    if (int rc = computed(b, true, "batch_get_landmark_variances_all")) return rc;
    const LmState &m = cov_of(b)->lm;
    const size_t nel = (size_t)b->in.n * m.lmax;
    if (!out || (long long)cap < (long long)nel) { set_error("batch_get_landmark_variances_all: the output array is missing or too small"); return TCV_ERR_INVALID; }
    std::vector<double> h(nel);
    if (nel > 0) if (int rc = tcv::staged_download(h.data(), m.d_var, sizeof(double) * nel, "download of the landmark variances")) return rc;
    for (int w = 0; w < b->in.n; w++) {
        const std::vector<int> &po = m.plan_of[w];
        double *o = out + (size_t)w * m.lmax;
        for (int l = 0; l < m.lmax; l++) o[l] = l < (int)po.size() ? h[(size_t)w * m.lmax + po[l]] : 0.0;
    }
    if (stride) *stride = m.lmax;
    return TCV_OK;
}
extern "C" int tcv_batch_get_landmark_cross(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols) {
    if (int rc = computed(b, true, "batch_get_landmark_cross")) return rc;
    const LmState &m = cov_of(b)->lm;
    const int n_cross = (int)m.res.req.size();
    if (window < 0 || window >= b->in.n || k < 0 || k >= n_cross) { set_error("batch_get_landmark_cross: window or cross block out of range"); return TCV_ERR_INVALID; }
    const std::vector<int> &po = m.plan_of[window];
    const int L = (int)po.size(), wk = m.res.cols[k];
    if (!out || (long long)cap < (long long)L * wk) { set_error("batch_get_landmark_cross: the output array is missing or too small"); return TCV_ERR_INVALID; }
    const int c0 = m.rq[(size_t)window * cov_rq_stride(n_cross) + RQ_REQ + 4 * k];      // first solved column of the block; -1: constant in this window
    std::vector<double> h((size_t)L * m.mstride);
    if (c0 >= 0 && !h.empty())
        if (int rc = tcv::staged_download(h.data(), m.d_cross + (size_t)window * m.lmax * m.mstride, sizeof(double) * h.size(), "download of the landmark cross covariance")) return rc;
    for (int l = 0; l < L; l++) for (int j = 0; j < wk; j++) out[(size_t)l * wk + j] = c0 >= 0 ? h[(size_t)po[l] * m.mstride + c0 + j] : 0.0;
    if (rows) *rows = L;
    if (cols) *cols = wk;
    return TCV_OK;
}
extern "C" int tcv_batch_landmark_covariance_status(tcv_batch *b, int *out, int n) {
    if (b && (!out || n != b->in.n)) { set_error("batch_landmark_covariance_status: n must be the batch size"); return TCV_ERR_INVALID; }
    if (int rc = computed(b, true, "batch_landmark_covariance_status")) return rc;
    return tcv::staged_download(out, cov_of(b)->lm.res.status, sizeof(int) * (size_t)n, "download of the landmark covariance status");
}
// one problem at the caller's current block values; the landmarks by address
extern "C" int tcv_problem_compute_landmark_covariance(tcv_problem *p, const tcv_covariance_options *o, double *const *inv_depth_addresses, int n,
                                                       const tcv_landmark_cross_block *cross, int n_cross, double *variances, double *const *cross_out,
                                                       int *status) {
    const char *who = "problem_compute_landmark_covariance";
    if (!p || !inv_depth_addresses || !variances) { set_error(std::string(who) + ": null problem, address list or variance array"); return TCV_ERR_INVALID; }
    if (n < 1) { set_error(std::string(who) + ": n must be at least 1"); return TCV_ERR_INVALID; }
    if (int rc = check_landmark(o, cross, n_cross, who)) return rc;
    if (n_cross > 0 && !cross_out) { set_error(std::string(who) + ": null cross output array with n_cross > 0"); return TCV_ERR_INVALID; }
    for (int k = 0; k < n_cross; k++) if (!cross_out[k]) { set_error(std::string(who) + ": null cross output block"); return TCV_ERR_INVALID; }
    if (o->at_solution) { set_error(std::string(who) + ": at_solution = 1 needs a solved batch (tcv_batch_compute_landmark_covariance)"); return TCV_ERR_INVALID; }
    if (int rc = check_requests(*p, diagonal_requests(cross, n_cross).data(), n_cross)) return rc;
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
    std::vector<double> var((size_t)std::max(1, L));      // the caller's memory is written only when everything came back
    std::vector<std::vector<double>> cr(n_cross);
    std::vector<int> wk(n_cross, 0);
    int st = 0;
    const int rc = one_window_batch(p, [&](tcv_batch *b) {
        int nl = 0, rc = tcv_batch_compute_landmark_covariance(b, o, cross, n_cross, TCV_STREAM_THREAD);
        if (rc == TCV_OK) rc = tcv_batch_get_landmark_variances(b, 0, var.data(), (int)var.size(), &nl);
        if (rc == TCV_OK && nl != L) { set_error(std::string(who) + ": the batch holds another number of landmarks than the problem"); rc = TCV_ERR_INVALID; }
        for (int k = 0; k < n_cross && rc == TCV_OK; k++) {
            int r = 0;
            cr[k].assign((size_t)std::max(1, L) * 9, 0.0);
            rc = tcv_batch_get_landmark_cross(b, 0, k, cr[k].data(), (int)cr[k].size(), &r, &wk[k]);
        }
        return rc == TCV_OK ? tcv_batch_landmark_covariance_status(b, &st, 1) : rc;
    });
    if (rc != TCV_OK) return rc;
    for (int i = 0; i < n; i++) variances[i] = var[which[i]];
    for (int k = 0; k < n_cross; k++) for (int i = 0; i < n; i++) std::memcpy(cross_out[k] + (size_t)i * wk[k], cr[k].data() + (size_t)which[i] * wk[k], sizeof(double) * wk[k]);
    if (status) *status = st;
    return TCV_OK;
}
