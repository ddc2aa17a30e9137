// Native estimator: what ONE estimator asks of the library around its window -- the 2D-3D line association (UpdateLinesInFoV /
// initialLineFoVWindow / updateLinePairInWindow, estimator.cpp:328-336, :385-497), the window description the problems are made from,
// the prior chain (getParameterBlocks, marginalization_factor.cpp:301-321) and the window tap with its snapshot getters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "tcv_est.h"
#include "tcv_runtime.h"       // set_error

using namespace tcv_est;

// the device-resident line map is bound to the device that was current at tcv_estimator_set_line_map: an estimator optimised with another
// current device uses the host copy it still holds (uploaded with the call) instead of failing the association (round-5 advisor finding)
extern "C" int tcv_line_map_device(const tcv_line_map *m);
static inline const tcv_line_map *map_on_current_device(const tcv_estimator *e) {
    if (!e->map_dev) return nullptr;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    return tcv_line_map_device(e->map_dev.get()) == cur ? e->map_dev.get() : nullptr;
}

namespace tcv_est {

int assoc_prepare(tcv_estimator *e, AssocJob &J) {
    poses_of(e, J.pose, J.ex);
    const int nm = e->n_map;
    for (auto &lf : e->linefeatures)
        for (size_t k = 0; k < lf.obs.size(); k++) { J.det_frame.push_back(lf.start + (int)k); J.det.insert(J.det.end(), lf.obs[k].vec, lf.obs[k].vec + 4); J.where.push_back(&lf.obs[k]); }
    J.one_call = e->fov_ready;      // steady state: UpdateLinesInFoV(frame_count) and the matching in ONE device call
    if (!e->fov_ready) {
        std::vector<unsigned char> fov_now((size_t)(W + 1) * nm, 0);
        const int rc = tcv_match_lines(W + 1, J.pose, J.ex, e->Rbw.data(), e->Tbw.data(), e->cfg.K, e->cfg.width, e->cfg.height, W, nm, e->map_lines.data(), 0, nullptr, nullptr,
                                       e->cfg.angle_th, e->cfg.overlap_th, 0, fov_now.data(), nullptr, nullptr, nullptr);
        if (rc != TCV_OK) return rc;
        for (int i = 0; i <= W; i++) e->fov[i].assign(fov_now.begin() + (size_t)i * nm, fov_now.begin() + (size_t)(i + 1) * nm);      // initialLineFoVWindow (:483-497)
        e->fov_ready = true;
    }
    J.given.assign((size_t)(W + 1) * nm, 0);
    for (int i = 0; i <= W; i++) if (!e->fov[i].empty()) std::copy(e->fov[i].begin(), e->fov[i].end(), J.given.begin() + (size_t)i * nm);
    const int nd = (int)J.where.size();
    J.match.assign(std::max(nd, 1), 0);
    J.err.assign((size_t)std::max(nd, 1) * 3, 0.0f);
    J.call = nd > 0 || J.one_call;
    tcv_match_lines_args &a = J.args;
    a.n_frames = W + 1; a.poses = J.pose; a.ex_pose = J.ex; a.Rbw = e->Rbw.data(); a.Tbw = e->Tbw.data(); a.K = e->cfg.K; a.width = e->cfg.width; a.height = e->cfg.height;
    a.window_size = W; a.n_map = nm; a.lines3d = e->map_lines.data(); a.map_device = map_on_current_device(e); a.n_det = nd; a.det_frame = nd ? J.det_frame.data() : nullptr; a.det_lines = nd ? J.det.data() : nullptr;
    a.angle_th = e->cfg.angle_th; a.overlap_th = e->cfg.overlap_th; a.fov_given = J.one_call ? 2 + W : 1; a.in_fov = J.given.data();
    a.match_index = nd ? J.match.data() : nullptr; a.err = nd ? J.err.data() : nullptr; a.projected = nullptr;
    return TCV_OK;
}
void assoc_finish(tcv_estimator *e, AssocJob &J) {
    const int nm = e->n_map, nd = (int)J.where.size();
    if (J.call && J.one_call) e->fov[W].assign(J.given.begin() + (size_t)W * nm, J.given.begin() + (size_t)(W + 1) * nm);                          // UpdateLinesInFoV(frame_count)
    for (int q = 0; q < nd; q++) {
        LineObs &ob = *J.where[q];
        ob.errA = (double)J.err[3 * q]; ob.errD = (double)J.err[3 * q + 1]; ob.overlap = (double)J.err[3 * q + 2];
        const unsigned char *g = J.given.data() + (size_t)J.det_frame[q] * nm;
        int first = -1;
        for (int i = 0; i < nm && first < 0; i++) if (g[i]) first = i;
        if (J.match[q] >= 0) std::memcpy(ob.world, e->map_lines.data() + 6 * J.match[q], sizeof ob.world);
        else if (first >= 0) std::memcpy(ob.world, e->map_lines.data() + 6 * first, sizeof ob.world);          // `linesInThisFov[0]` (:871-877)
        else { const double fake[6] = {ob.vec[0], ob.vec[1], 1.0, ob.vec[0], ob.vec[1], 1.0}; std::memcpy(ob.world, fake, sizeof fake); }      // fake_line (:707-709)
        ob.use_flag = true;
        ob.credible_line = J.err[3 * q] != -1.0f;
    }
    remove_line_outlier(e);
}

// the window (marg: its marginalisation problem, whose lists build_marg left empty for MARGIN_SECOND_NEW) as tcv_problem_from_window takes it
void fill_desc(tcv_estimator *e, tcv_window_desc &d, bool marg) {
    std::memset(&d, 0, sizeof d);
    d.n_frames = W + 1; d.n_landmarks = (int)e->sel.size(); d.estimate_extrinsic = e->cfg.estimate_extrinsic;
    d.para_pose = e->para_pose; d.para_speedbias = e->para_sb; d.para_ex_pose = e->para_ex; d.para_feature = e->para_feature.data();
    d.proj_sqrt_info = e->cfg.focal_length / 1.5; d.proj_loss_a = 1.0; d.line_loss_a = 1.0;
    std::memcpy(d.line_K, e->cfg.K, sizeof d.line_K); std::memcpy(d.line_Ric, e->w_Ric, sizeof d.line_Ric);
    for (int c = 0; c < 3; c++) { d.line_Tic[c] = e->tic[c]; d.gravity[c] = e->cfg.gravity[c]; }
    d.line_exact_jacobian = e->cfg.line_exact_jacobian;
    d.prior = e->prior; d.prior_block_kind = e->w_pk.data(); d.prior_block_index = e->w_pidx.data();
    if (e->estimate_td) { d.para_td = e->para_td; d.td_TR = e->td_TR; d.td_ROW = e->td_ROW; }      // :1703-1707
    (marg ? e->m : e->w).bind(d, e->estimate_td != 0);
}

// getParameterBlocks(addr_shift) (marginalization_factor.cpp:301-321; estimator.cpp:2027-2039 / :2084-2104)
int take_prior(tcv_estimator *e, tcv_prior *np, int flag) {
    int m, n, nb, xs;
    int rc = tcv_prior_dims(np, &m, &n, &nb, &xs);
    if (rc != TCV_OK) return rc;
    std::vector<double *> addr(nb);
    rc = tcv_prior_keep_block_addresses(np, addr.data());
    if (rc != TCV_OK) return rc;
    std::vector<std::pair<int, int>> blocks;
    for (int k = 0; k < nb; k++) {
        int kind = -1, idx = 0;
        if (addr[k] >= e->para_pose && addr[k] < e->para_pose + (W + 1) * 7) { kind = 0; idx = (int)(addr[k] - e->para_pose) / 7; }
        else if (addr[k] >= e->para_sb && addr[k] < e->para_sb + (W + 1) * 9) { kind = 1; idx = (int)(addr[k] - e->para_sb) / 9; }
        else if (addr[k] == e->para_ex) { kind = 2; idx = 0; }
        else if (e->estimate_td && addr[k] == e->para_td) { kind = 3; idx = 0; }      // addr_shift[para_Td[0]] = para_Td[0] (:2035-2038, :2101-2104)
        else { tcv::set_error("estimator: kept block is not a pose / speed-bias / extrinsic / time-offset block"); return TCV_ERR_INVALID; }
        if (kind < 2) {
            if (flag == MARGIN_OLD) idx -= 1;
            else if (idx == W) idx -= 1;
        }
        blocks.push_back({kind, idx});
    }
    if (e->prior) tcv_prior_destroy(e->prior);
    e->prior = np;
    e->prior_blocks = blocks;
    e->stats.prior_n = n;
    return TCV_OK;
}

// the window build_window() just made, copied for the tap (device-resident inputs are materialised: tcv_preint_export / tcv_prior_export)
int tap_window(tcv_estimator *e) {
    WindowTap &T = e->tap;
    T.have = false; T.applied = 0; T.iterations = 0; T.final_cost = 0;
    T.pose_in.assign(e->para_pose, e->para_pose + (W + 1) * 7); T.sb_in.assign(e->para_sb, e->para_sb + (W + 1) * 9);
    T.ex_in.assign(e->para_ex, e->para_ex + 7); T.feat_in.assign(e->para_feature.begin(), e->para_feature.begin() + e->sel.size());
    T.pose_out.assign((W + 1) * 7, 0.0); T.sb_out.assign((W + 1) * 9, 0.0); T.ex_out.assign(7, 0.0); T.feat_out.assign(e->sel.size(), 0.0);
    T.f = e->w;
    for (size_t k = 0; k < T.f.imu.size(); k++)
        if (T.f.imu_dev[k]) { const int rc = tcv_preint_export(T.f.imu_dev[k], &T.f.imu[k]); if (rc != TCV_OK) return rc; }
    T.f.imu_dev.clear();      // (the handles are the window's: the snapshot holds the numbers)
    T.td_in = e->estimate_td ? e->para_td[0] : 0.0; T.td_out = 0.0;
    T.has_relo = e->w_relo; T.r_pi = e->r_pi; T.r_pl = e->r_pl; T.r_pts = e->r_pts;
    T.relo_local = e->w_relo_local; T.relo_frame_index = e->w_relo_frame_index; T.relo_frame_serial = e->w_relo_serial;
    std::memset(T.relo_out, 0, sizeof T.relo_out); std::memset(&T.relo_result, 0, sizeof T.relo_result);
    if (e->w_relo) { std::memcpy(T.relo_in, e->relo_pose, sizeof T.relo_in); std::memcpy(T.relo_prev, e->w_relo_prev, sizeof T.relo_prev); }
    else { std::memset(T.relo_in, 0, sizeof T.relo_in); std::memset(T.relo_prev, 0, sizeof T.relo_prev); }
    std::memcpy(T.Ric, e->w_Ric, sizeof T.Ric);
    T.marg_flag = e->marg_flag;
    T.pk = e->w_pk; T.pidx = e->w_pidx; T.psize.clear(); T.pcol.clear(); T.x0.clear(); T.J0.clear(); T.r0.clear();
    T.prior_m = T.prior_n = 0;
    if (e->prior) {
        int m, nn, nb, xs;
        int rc = tcv_prior_dims(e->prior, &m, &nn, &nb, &xs);
        if (rc != TCV_OK) return rc;
        T.psize.resize(nb); T.pcol.resize(nb); T.x0.resize(xs); T.J0.resize((size_t)nn * nn); T.r0.resize(nn);
        rc = tcv_prior_export(e->prior, T.psize.data(), T.pcol.data(), T.x0.data(), T.J0.data(), T.r0.data());
        if (rc != TCV_OK) return rc;
        T.prior_m = m; T.prior_n = nn;
    }
    T.have = true;
    return TCV_OK;
}

}  // namespace tcv_est

// the tap's snapshot, or null with the error text set: tap off, or no window optimised since it was switched on
static const WindowTap *snapshot_of(const tcv_estimator *e, const void *out, const char *who) {
    if (!e || !out) return nullptr;
    if (e->tap.on && e->tap.have) return &e->tap;
    tcv::set_error(std::string(who) + ": no snapshot (tap off, or no window optimised since it was switched on)");
    return nullptr;
}
extern "C" int tcv_estimator_get_window_snapshot(const tcv_estimator *e, tcv_window_snapshot *o) {
    const WindowTap *tp = snapshot_of(e, o, "estimator_get_window_snapshot");
    if (!tp) return TCV_ERR_INVALID;
    const WindowTap &T = *tp;
    std::memset(o, 0, sizeof *o);
    o->n_frames = W + 1; o->n_landmarks = (int)T.feat_in.size();
    T.f.bind_lists(*o);
    o->marg_flag = T.marg_flag; o->estimate_extrinsic = e->cfg.estimate_extrinsic; o->line_exact_jacobian = e->cfg.line_exact_jacobian;
    o->pose_in = T.pose_in.data(); o->speedbias_in = T.sb_in.data(); o->ex_pose_in = T.ex_in.data(); o->feature_in = T.feat_in.data();
    o->pose_out = T.pose_out.data(); o->speedbias_out = T.sb_out.data(); o->ex_pose_out = T.ex_out.data(); o->feature_out = T.feat_out.data();
    std::memcpy(o->line_K, e->cfg.K, sizeof o->line_K); std::memcpy(o->line_Ric, T.Ric, sizeof o->line_Ric);
    for (int c = 0; c < 3; c++) { o->line_Tic[c] = T.ex_in[c]; o->gravity[c] = e->cfg.gravity[c]; }
    o->proj_sqrt_info = e->cfg.focal_length / 1.5;
    o->prior_m = T.prior_m; o->prior_n = T.prior_n; o->prior_nblk = (int)T.psize.size();
    o->prior_block_kind = T.pk.data(); o->prior_block_index = T.pidx.data(); o->prior_block_size = T.psize.data(); o->prior_block_idx = T.pcol.data();
    o->prior_x0 = T.x0.data(); o->prior_J0 = T.J0.data(); o->prior_r0 = T.r0.data();
    o->iterations = T.iterations; o->applied = T.applied; o->final_cost = T.final_cost;
    return TCV_OK;
}
extern "C" int tcv_estimator_get_window_snapshot_td(const tcv_estimator *e, tcv_window_snapshot_td *o) {
    const WindowTap *tp = snapshot_of(e, o, "estimator_get_window_snapshot_td");
    if (!tp) return TCV_ERR_INVALID;
    const WindowTap &T = *tp;
    std::memset(o, 0, sizeof *o);
    o->estimate_td = e->estimate_td; o->n_proj = (int)T.f.pi.size();
    o->td_in = T.td_in; o->td_out = T.td_out; o->TR = e->td_TR; o->ROW = e->td_ROW;
    o->proj_td_aux = T.f.aux.empty() ? nullptr : T.f.aux.data();
    return TCV_OK;
}
extern "C" int tcv_estimator_get_window_snapshot_relo(const tcv_estimator *e, tcv_window_snapshot_relo *o) {
    const WindowTap *tp = snapshot_of(e, o, "estimator_get_window_snapshot_relo");
    if (!tp) return TCV_ERR_INVALID;
    const WindowTap &T = *tp;
    std::memset(o, 0, sizeof *o);
    if (!T.has_relo) return TCV_OK;
    o->has_relo = 1; o->local_index = T.relo_local; o->n_relo = (int)T.r_pi.size(); o->frame_index = T.relo_frame_index; o->frame_serial = T.relo_frame_serial;
    std::memcpy(o->relo_pose_in, T.relo_in, sizeof o->relo_pose_in); std::memcpy(o->relo_pose_out, T.relo_out, sizeof o->relo_pose_out);
    o->relo_frame_i = T.r_pi.data(); o->relo_feature = T.r_pl.data(); o->relo_pts = T.r_pts.data();
    std::memcpy(o->prev_relo_t, T.relo_prev, sizeof o->prev_relo_t); std::memcpy(o->prev_relo_r, T.relo_prev + 3, sizeof o->prev_relo_r);
    o->result = T.relo_result;
    return TCV_OK;
}
