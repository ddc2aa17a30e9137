// Host half of ceres::Problem::Evaluate on a resident batch (include/tcv.h tcv_batch_evaluate; the kernel: tcv_eval.hip): the owner
// lists of the gradient, the evaluation buffers of a batch and the getters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tcv_eval.h"
#include "tcv_host.h"

using namespace tcv;

// =====================================================================================================
// ceres::Problem::Evaluate on a resident batch (tcv_eval.hip)
// =====================================================================================================
extern "C" int tcv_launch_evaluate(const tcv::EvalArgs *args, size_t lds_bytes, void *stream);
namespace {
struct EvalState : tcv::SideState {
    PlanTable tab;              // the owner lists of every plan
    void *d_out = nullptr;      // [scalars | residuals | block costs | gradient | staging], per window each
    double *d_scal = nullptr, *d_res = nullptr, *d_blk = nullptr, *d_grad = nullptr, *d_stage = nullptr;
    int res_stride = 0, blk_stride = 0, grad_stride = 0, stage_stride = 0;
    bool evaluated = false;
    tcv_evaluate_options last;
    ~EvalState() override { tcv::dev_free(tab.d); tcv::dev_free(d_out); }
};
EvalState *eval_of(const tcv_batch *b) { return static_cast<EvalState *>(b->eval.get()); }
}  // namespace
// Owner lists of the gradient for the plan of window w (tcv_eval.h): per tangent index (camera tangent space, then the landmarks) the
// offsets of its J'r pieces in the window's piece region, in factor order -- prior, IMU, point (plan order), line.  A function of the
// plan's tables alone (block table, factor tables, prior columns), rebuilt here from the problem the plan was packed from.
static void eval_owner_lists(const tcv_batch *b, int w, std::vector<int> &out) {
    const tcv_problem &p = *b->in.problems[w];
    const Packed &pk = b->in.packed[w];
    const PlanHdr &H = b->in.plans[b->in.wins[w].plan];
    const int nl = H.nc + H.nland;
    const BlockMap map(p, pk);
    std::vector<std::vector<int>> own(nl);
    int off = 0;
    if (H.prior_n > 0) {
        const tcv_prior *pr = p.prior[0].prior;
        for (int k = 0; k < H.prior_nblk; k++) {
            const int t = map.toff(p.prior[0].b[k]), local = pr->size[k] == 7 ? 6 : pr->size[k];
            for (int j = 0; j < local; j++) if (t >= 0 && pr->idx[k] + j < pr->n) own[t + j].push_back(off + pr->idx[k] + j);
        }
        off += H.prior_n;
    }
    for (size_t f = 0; f < p.imu.size(); f++) {
        static const int col0[4] = {0, 6, 15, 21}, wid[4] = {6, 9, 6, 9};
        for (int k = 0; k < 4; k++) {
            const int t = map.toff(p.imu[f].b[k]);
            for (int j = 0; j < wid[k]; j++) if (t >= 0) own[t + j].push_back(off + (int)f * EV_PIECE_IMU + col0[k] + j);
        }
    }
    off += EV_PIECE_IMU * H.n_imu;
    for (size_t k = 0; k < pk.proj_order.size(); k++) {
        const ProjFac &f = p.proj[pk.proj_order[k]];
        for (int s = 0; s < 3; s++) {
            const int t = map.toff(f.b[s]);
            for (int j = 0; j < 6; j++) if (t >= 0) own[t + j].push_back(off + (int)k * EV_PIECE_PROJ + 6 * s + j);
        }
        own[H.nc + map.lm_of(f.b[3])].push_back(off + (int)k * EV_PIECE_PROJ + 18);
        if (f.btd >= 0) { const int t = map.toff(f.btd); if (t >= 0) own[t].push_back(off + (int)k * EV_PIECE_PROJ + 19); }
    }
    off += EV_PIECE_PROJ * H.n_proj;
    for (size_t k = 0; k < p.line.size(); k++) {
        const int t = map.toff(p.line[k].b);
        for (int j = 0; j < 6; j++) if (t >= 0) own[t + j].push_back(off + (int)k * EV_PIECE_LINE + j);
    }
    out.clear();
    int e = 0;
    for (int t = 0; t < nl; t++) { out.push_back(e); e += (int)own[t].size(); }
    out.push_back(e);
    for (int t = 0; t < nl; t++) out.insert(out.end(), own[t].begin(), own[t].end());
}
// first evaluation of a batch: the owner lists of its distinct plans go up, staging and output buffers are allocated (returned by tcv_batch_destroy)
static int eval_prepare(tcv_batch *b) {
    if (b->eval) return TCV_OK;
    std::unique_ptr<EvalState> s(new EvalState());
    const int n = b->in.n;
    for (auto &H : b->in.plans) {
        s->res_stride = std::max(s->res_stride, eval_num_residuals(H)); s->blk_stride = std::max(s->blk_stride, eval_num_blocks(H));
        s->stage_stride = std::max(s->stage_stride, (eval_stage_doubles(H) + 1) & ~1);
    }
    s->res_stride = (s->res_stride + 1) & ~1; s->blk_stride = (s->blk_stride + 1) & ~1; s->grad_stride = b->in.delta_stride;
    const size_t per_win = (size_t)EV_SCALARS + s->res_stride + s->blk_stride + s->grad_stride + s->stage_stride;
    if (int rc = plan_table_create(b, [&](int w, std::vector<int> &out) { eval_owner_lists(b, w, out); return (int)TCV_OK; },
                                   "hipMalloc (evaluation buffers)", "upload of the evaluation tables", &s->tab)) return rc;
    if (hipError_t e = tcv::dev_malloc(&s->d_out, sizeof(double) * per_win * (size_t)n)) { tcv::dev_free(s->tab.d); return hip_fail(e, "hipMalloc (evaluation buffers)"); }
    s->d_scal = (double *)s->d_out; s->d_res = s->d_scal + (size_t)n * EV_SCALARS; s->d_blk = s->d_res + (size_t)n * s->res_stride;
    s->d_grad = s->d_blk + (size_t)n * s->blk_stride; s->d_stage = s->d_grad + (size_t)n * s->grad_stride;
    b->eval = std::move(s);
    return TCV_OK;
}
extern "C" void tcv_evaluate_options_default(tcv_evaluate_options *o) {
    if (!o) return;
    o->at = TCV_EVALUATE_AT_INITIAL;
    o->apply_loss_function = 1;
    o->want_residuals = o->want_gradient = o->want_block_costs = 0;
}
// Problem::Evaluate(options, &cost, &residuals, &gradient, nullptr) for every window of the batch
extern "C" int tcv_batch_evaluate(tcv_batch *b, const tcv_evaluate_options *o, void *hip_stream) {
    if (!b || !o) { set_error("batch_evaluate: null batch or options"); return TCV_ERR_INVALID; }
    if (o->at != TCV_EVALUATE_AT_INITIAL && o->at != TCV_EVALUATE_AT_SOLUTION) { set_error("batch_evaluate: options.at must be TCV_EVALUATE_AT_INITIAL or TCV_EVALUATE_AT_SOLUTION"); return TCV_ERR_INVALID; }
    if (o->at == TCV_EVALUATE_AT_SOLUTION && !b->last.solved) { set_error("batch_evaluate: at = solution, but the batch has not been solved"); return TCV_ERR_INVALID; }
    hip_stream = (void *)tcv::resolve_stream(hip_stream);
    if (int rc = eval_prepare(b)) return rc;
    EvalState *s = eval_of(b);
    EvalArgs a;
    std::memset(&a, 0, sizeof a);
    a.win = b->mem.d_win; a.plans = b->mem.d_plans; a.plan_base = b->mem.d_plan_base; a.ipool = b->mem.d_ipool; a.dpool = b->mem.d_dpool;
    a.state = o->at == TCV_EVALUATE_AT_SOLUTION ? b->mem.d_state : nullptr;
    a.tab_base = s->tab.base; a.tab = s->tab.ints;
    a.scalars = s->d_scal;
    a.residuals = o->want_residuals ? s->d_res : nullptr; a.block_cost = o->want_block_costs ? s->d_blk : nullptr;
    a.gradient = o->want_gradient ? s->d_grad : nullptr; a.stage = s->d_stage;
    a.nwin = b->in.n; a.state_stride = b->in.state_stride; a.res_stride = s->res_stride; a.blk_stride = s->blk_stride;
    a.grad_stride = s->grad_stride; a.stage_stride = s->stage_stride;
    a.apply_loss = o->apply_loss_function ? 1 : 0;
    if (int rc = b->flight.enter((hipStream_t)hip_stream)) return rc;
    const int rc = tcv_launch_evaluate(&a, sizeof(double) * (size_t)eval_lds_doubles(b->in.state_stride), hip_stream);
    if (rc != 0) return hip_fail((hipError_t)rc, "evaluate kernel launch");
    s->evaluated = true; s->last = *o;
    return TCV_OK;
}
static int eval_local_size(const tcv_batch *b, int window) {
    const tcv_problem &p = *b->in.problems[window];
    const Packed &pk = b->in.packed[window];
    int k = 0;
    for (size_t c = 0; c < pk.cam_block.size(); c++)
        if (pk.cam_loff[c] >= 0) { const ParamBlock &pb = p.blocks[pk.cam_block[c]]; k += pb.kind == KIND_POSE ? 6 : pb.size; }
    return k + b->in.plans[b->in.wins[window].plan].nland;
}
extern "C" int tcv_batch_evaluation_dims(const tcv_batch *b, int window, int *num_residuals, int *num_residual_blocks, int *num_local) {
    if (!b || window < 0 || window >= b->in.n) { set_error("batch_evaluation_dims: no batch / window out of range"); return TCV_ERR_INVALID; }
    const PlanHdr &H = b->in.plans[b->in.wins[window].plan];
    if (num_residuals) *num_residuals = eval_num_residuals(H);
    if (num_residual_blocks) *num_residual_blocks = eval_num_blocks(H) - 1 + (int)b->in.problems[window]->prior.size();
    if (num_local) *num_local = eval_local_size(b, window);
    return TCV_OK;
}
static int eval_ready(tcv_batch *b, const char *who) {
    if (!b) { set_error(std::string(who) + ": null batch"); return TCV_ERR_INVALID; }
    if (!eval_of(b) || !eval_of(b)->evaluated) { set_error(std::string(who) + ": the batch has not been evaluated"); return TCV_ERR_INVALID; }
    return b->settle();
}
static bool eval_finite(const double *v, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }
extern "C" int tcv_batch_get_evaluation(tcv_batch *b, int window, double *cost, double family_cost[4], double *gradient_max_norm,
                                        double *residuals, int residuals_cap, double *block_costs, int block_costs_cap, double *gradient,
                                        int gradient_cap) {
    if (b && (window < 0 || window >= b->in.n)) { set_error("batch_get_evaluation: window out of range"); return TCV_ERR_INVALID; }
    if (int rc = eval_ready(b, "batch_get_evaluation")) return rc;
    EvalState *s = eval_of(b);
    if ((residuals && !s->last.want_residuals) || (block_costs && !s->last.want_block_costs) || (gradient && !s->last.want_gradient)) {
        set_error("batch_get_evaluation: an output the last tcv_batch_evaluate was not asked for"); return TCV_ERR_INVALID;
    }
    const PlanHdr &H = b->in.plans[b->in.wins[window].plan];
    const tcv_problem &p = *b->in.problems[window];
    const Packed &pk = b->in.packed[window];
    const int nres = eval_num_residuals(H), nblk = eval_num_blocks(H) - 1 + (int)p.prior.size(), nloc = eval_local_size(b, window);
    if ((residuals && residuals_cap < nres) || (block_costs && block_costs_cap < nblk) || (gradient && gradient_cap < nloc)) {
        set_error("batch_get_evaluation: an output array is too small (tcv_batch_evaluation_dims)"); return TCV_ERR_INVALID;
    }
    // one staged copy: [scalars | residuals | block costs | gradient] of the window, the parts that were asked for
    const size_t o_res = EV_SCALARS, o_blk = o_res + (residuals ? s->res_stride : 0), o_grad = o_blk + (block_costs ? s->blk_stride : 0);
    std::vector<double> h(o_grad + (gradient ? s->grad_stride : 0));
    if (int rc = tcv::staged_download(h.data(), s->d_scal + (size_t)window * EV_SCALARS, sizeof(double) * EV_SCALARS, "download of the evaluation")) return rc;
    if (residuals) if (int rc = tcv::staged_download(h.data() + o_res, s->d_res + (size_t)window * s->res_stride, sizeof(double) * nres, "download of the evaluation")) return rc;
    if (block_costs) if (int rc = tcv::staged_download(h.data() + o_blk, s->d_blk + (size_t)window * s->blk_stride, sizeof(double) * eval_num_blocks(H), "download of the evaluation")) return rc;
    if (gradient) if (int rc = tcv::staged_download(h.data() + o_grad, s->d_grad + (size_t)window * s->grad_stride, sizeof(double) * (H.nc + H.nland), "download of the evaluation")) return rc;
    bool ok = eval_finite(h.data(), 5) && (!gradient || eval_finite(h.data() + EV_GMAX, 1));
    if (cost) *cost = h[EV_COST];
    if (family_cost) for (int k = 0; k < 4; k++) family_cost[k] = h[EV_FAMILY + k];
    if (gradient_max_norm) *gradient_max_norm = h[EV_GMAX];
    // the point factors come back in plan order (sorted by landmark): proj_order[k] is the caller's index of the k-th
    const int r_proj = H.prior_n + 15 * H.n_imu, r_line = r_proj + 2 * H.n_proj;
    if (residuals) {
        const double *r = h.data() + o_res;
        std::memcpy(residuals, r, sizeof(double) * r_proj);
        for (int k = 0; k < H.n_proj; k++) { const int f = pk.proj_order[k]; residuals[r_proj + 2 * f] = r[r_proj + 2 * k]; residuals[r_proj + 2 * f + 1] = r[r_proj + 2 * k + 1]; }
        std::memcpy(residuals + r_line, r + r_line, sizeof(double) * 2 * H.n_line);
        ok = ok && eval_finite(residuals, nres);
    }
    if (block_costs) {
        const double *c = h.data() + o_blk;
        int k0 = 0;
        if (!p.prior.empty()) block_costs[k0++] = c[0];
        for (int f = 0; f < H.n_imu; f++) block_costs[k0 + f] = c[1 + f];
        for (int k = 0; k < H.n_proj; k++) block_costs[k0 + H.n_imu + pk.proj_order[k]] = c[1 + H.n_imu + k];
        for (int f = 0; f < H.n_line; f++) block_costs[k0 + H.n_imu + H.n_proj + f] = c[1 + H.n_imu + H.n_proj + f];
    }
    if (gradient) {      // the layout of tcv_batch_get_first_step
        const double *g = h.data() + o_grad;
        int k = 0;
        for (size_t c = 0; c < pk.cam_block.size(); c++) {
            if (pk.cam_loff[c] < 0) continue;
            const ParamBlock &pb = p.blocks[pk.cam_block[c]];
            const int ls = pb.kind == KIND_POSE ? 6 : pb.size;
            for (int j = 0; j < ls; j++) gradient[k++] = g[pk.cam_loff[c] + j];
        }
        for (int l = 0; l < H.nland; l++) gradient[k++] = g[H.nc + l];
    }
    if (!ok) { set_error("batch_get_evaluation: NaN / Inf in the evaluation"); return TCV_ERR_NUMERIC; }
    return TCV_OK;
}
extern "C" int tcv_batch_get_evaluation_costs(tcv_batch *b, double *cost, double *family_cost, double *gradient_max_norm, int n) {
    if (b && n != b->in.n) { set_error("batch_get_evaluation_costs: n must be the batch size"); return TCV_ERR_INVALID; }
    if (int rc = eval_ready(b, "batch_get_evaluation_costs")) return rc;
    EvalState *s = eval_of(b);
    std::vector<double> h((size_t)n * EV_SCALARS);
    if (int rc = tcv::staged_download(h.data(), s->d_scal, sizeof(double) * h.size(), "download of the evaluation")) return rc;
    bool ok = true;
    for (int w = 0; w < n; w++) {
        const double *q = h.data() + (size_t)w * EV_SCALARS;
        if (cost) cost[w] = q[EV_COST];
        if (family_cost) for (int k = 0; k < 4; k++) family_cost[4 * w + k] = q[EV_FAMILY + k];
        if (gradient_max_norm) gradient_max_norm[w] = q[EV_GMAX];
        ok = ok && eval_finite(q, 6);
    }
    if (!ok) { set_error("batch_get_evaluation_costs: NaN / Inf in the evaluation"); return TCV_ERR_NUMERIC; }
    return TCV_OK;
}
extern "C" int tcv_problem_num_effective_parameters(const tcv_problem *p) {
    if (!p) return 0;
    int k = 0;
    for (auto &pb : p->blocks) if (!pb.constant) k += pb.kind == KIND_POSE ? 6 : pb.size;
    return k;
}
// Problem::Evaluate for one problem at the caller's current block values: a one-window batch evaluated at its initial state
extern "C" int tcv_problem_evaluate(tcv_problem *p, const tcv_evaluate_options *o, double *cost, double *residuals, double *gradient, double *family_cost) {
    if (!p || !o) { set_error("problem_evaluate: null problem or options"); return TCV_ERR_INVALID; }
    tcv_batch *b = nullptr;
    tcv_problem *arr[1] = {p};
    int rc = tcv_batch_create(&b, arr, nullptr, nullptr, nullptr, 1);
    if (rc != TCV_OK) return rc;
    tcv_evaluate_options eo = *o;
    eo.at = TCV_EVALUATE_AT_INITIAL; eo.want_residuals = residuals != nullptr; eo.want_gradient = gradient != nullptr; eo.want_block_costs = 0;
    rc = tcv_batch_evaluate(b, &eo, TCV_STREAM_THREAD);
    int nres = 0, nloc = 0;
    if (rc == TCV_OK) rc = tcv_batch_evaluation_dims(b, 0, &nres, nullptr, &nloc);
    if (rc == TCV_OK) rc = tcv_batch_get_evaluation(b, 0, cost, family_cost, nullptr, residuals, nres, nullptr, 0, gradient, nloc);
    tcv_batch_destroy(b);
    return rc;
}
