// Native mirror of the estimator's per-frame window management around the hot path (include/tcv_estimator.h): the C-ABI
// of ONE estimator -- create, reset, destroy, the setters, begin_frame (processIMU + processImagewithLine up to solveOdometry,
// estimator.cpp:191-383), finish_frame and their batched forms.  The state is tcv_est.h, the bookkeeping tcv_est_tracks.cpp, the window's
// calls into the library tcv_est_window.cpp, the lock-step frame tcv_est_lockstep.cpp.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tcv_est.h"
#include "tcv_runtime.h"       // set_error

using namespace tcv_est;

// every part but the settings and the tap afresh (tcv_est.h), then what derives from the settings
static void reset_state(tcv_estimator *e) {
    if (e->prior) tcv_prior_destroy(e->prior);
    e->fresh<EstStates>(); e->fresh<EstImu>(); e->fresh<EstTracks>(); e->fresh<EstWindow>(); e->fresh<EstPriorChain>(); e->fresh<EstTd>(); e->fresh<EstRelo>(); e->fresh<EstFrame>();
    for (int c = 0; c < 3; c++) e->tic[c] = e->cfg.tic[c];
    std::memcpy(e->ric.data(), e->cfg.ric, sizeof(double) * 9);
    e->td = e->td0; e->para_td[0] = e->td0;      // td = TD (estimator.cpp:51, :170)
}
extern "C" int tcv_estimator_create(tcv_estimator **out, const tcv_estimator_config *cfg) {
    if (!out || !cfg || !(cfg->imu_dt > 0) || !(cfg->focal_length > 0) || cfg->num_iterations < 1) { tcv::set_error("estimator_create: bad configuration"); return TCV_ERR_INVALID; }
    tcv_estimator *e = new tcv_estimator();
    e->cfg = *cfg;
    reset_state(e);
    *out = e;
    return TCV_OK;
}
// Estimator::clearState() + setParameter() (estimator.cpp:126-189, :39-52): what estimator_node.cpp does after failureDetection fired
// (:437-446) or on a restart request -- window, IMU buffers, pre-integrations, feature and line tracks, the marginalisation prior and the
// biases are dropped, the extrinsic goes back to the configured one; the line map (setParameters, :54-124) stays.
extern "C" int tcv_estimator_reset(tcv_estimator *e) {
    if (!e) return TCV_ERR_INVALID;
    reset_state(e);
    return TCV_OK;
}
extern "C" void tcv_estimator_destroy(tcv_estimator *e) {
    if (!e) return;
    if (e->prior) tcv_prior_destroy(e->prior);
    delete e;
}
extern "C" int tcv_estimator_set_biases(tcv_estimator *e, const double ba[3], const double bg[3]) {
    if (!e || !ba || !bg) return TCV_ERR_INVALID;
    for (int i = 0; i <= W; i++) for (int c = 0; c < 3; c++) { e->Bas[i][c] = ba[c]; e->Bgs[i][c] = bg[c]; }
    return TCV_OK;
}
extern "C" int tcv_estimator_set_line_map(tcv_estimator *e, int n, const double *lines3d, const double Rbw[9], const double Tbw[3]) {
    if (!e || n <= 0 || !lines3d || !Rbw || !Tbw) { tcv::set_error("estimator_set_line_map: bad argument"); return TCV_ERR_INVALID; }
    e->assoc = true; e->n_map = n;
    e->map_lines.assign(lines3d, lines3d + (size_t)6 * n);
    {      // (best effort: without the handle the association uploads the map per call, same results)
        tcv_line_map *md = nullptr;
        e->map_dev.reset();
        if (!getenv("TCV_EST_HOST_MAP") && tcv_line_map_create(&md, n, lines3d) == TCV_OK) e->map_dev = std::shared_ptr<tcv_line_map>(md, tcv_line_map_destroy);
    }
    std::memcpy(e->Rbw.data(), Rbw, sizeof(double) * 9);
    for (int c = 0; c < 3; c++) e->Tbw[c] = Tbw[c];
    return TCV_OK;
}

extern "C" int tcv_estimator_set_time_offset(tcv_estimator *e, int estimate_td, double td0, double TR, double ROW) {
    if (!e) { tcv::set_error("estimator_set_time_offset: bad argument"); return TCV_ERR_INVALID; }
    if (!(ROW > 0.0) || !std::isfinite(ROW) || !std::isfinite(td0) || !std::isfinite(TR)) { tcv::set_error("estimator_set_time_offset: ROW must be positive (and ROW, td0, TR finite)"); return TCV_ERR_INVALID; }
    if (e->frame_count != 0 || e->phase != 0 || !e->features.empty()) { tcv::set_error("estimator_set_time_offset: only while the window is empty (after create or reset)"); return TCV_ERR_INVALID; }
    e->estimate_td = estimate_td != 0; e->td0 = td0; e->td = td0; e->para_td[0] = td0; e->td_TR = TR; e->td_ROW = ROW;
    return TCV_OK;
}
extern "C" int tcv_estimator_stage_point_aux(tcv_estimator *e, int n_points, const double *aux4) {
    if (!e || n_points < 0 || (n_points > 0 && !aux4)) { tcv::set_error("estimator_stage_point_aux: bad argument"); return TCV_ERR_INVALID; }
    if (aux4) e->staged_aux.assign(aux4, aux4 + (size_t)4 * n_points); else e->staged_aux.clear();
    e->staged_n = n_points;
    return TCV_OK;
}
extern "C" int tcv_estimator_get_time_offset(const tcv_estimator *e, double *td) {
    if (!e || !td) { tcv::set_error("estimator_get_time_offset: bad argument"); return TCV_ERR_INVALID; }
    *td = e->td;
    return TCV_OK;
}

extern "C" int tcv_estimator_frame_serial(const tcv_estimator *e, int *next_serial, int *window_serials, int *n_slots) {
    if (!e) { tcv::set_error("estimator_frame_serial: bad argument"); return TCV_ERR_INVALID; }
    if (next_serial) *next_serial = e->next_serial;
    int n = 0;
    for (int i = 0; i <= W; i++) { if (window_serials) window_serials[i] = e->serials[i]; n += e->serials[i] >= 0 ? 1 : 0; }
    if (n_slots) *n_slots = n;
    return TCV_OK;
}
// Estimator::setReloFrame (estimator.cpp:2261-2279)
extern "C" int tcv_estimator_set_relo_frame(tcv_estimator *e, int frame_serial, int frame_index, int n_match, const double *match_points,
                                            const double prev_relo_t[3], const double prev_relo_r[9], int *accepted) {
    if (accepted) *accepted = 0;
    if (!e || !accepted || n_match < 0 || (n_match > 0 && !match_points) || !prev_relo_t || !prev_relo_r) { tcv::set_error("estimator_set_relo_frame: bad argument"); return TCV_ERR_INVALID; }
    if (e->phase != 0) { tcv::set_error("estimator_set_relo_frame: only between frames (after finish_frame, before the next begin_frame)"); return TCV_ERR_INVALID; }
    if (e->estimate_td) { tcv::set_error("estimator_set_relo_frame: not with estimate_td on (a problem holds either ProjectionFactors or ProjectionTdFactors)"); return TCV_ERR_INVALID; }
    for (int k = 0; k < 3 * n_match; k++) if (!std::isfinite(match_points[k])) { tcv::set_error("estimator_set_relo_frame: match_points not finite"); return TCV_ERR_INVALID; }
    for (int k = 1; k < n_match; k++)
        if (!((int)match_points[3 * k + 2] > (int)match_points[3 * k - 1])) { tcv::set_error("estimator_set_relo_frame: match_points must be strictly ascending in feature id"); return TCV_ERR_INVALID; }
    for (int k = 0; k < 12; k++) if (!std::isfinite(k < 3 ? prev_relo_t[k] : prev_relo_r[k - 3])) { tcv::set_error("estimator_set_relo_frame: prev_relo_t / prev_relo_r not finite"); return TCV_ERR_INVALID; }
    if (frame_serial < 0) return TCV_OK;
    for (int i = 0; i < W; i++) {      // :2269: the newest slot is not searched
        if (e->serials[i] != frame_serial) continue;
        e->relo_pending = true; e->relo_serial = frame_serial; e->relo_frame_index = frame_index; e->relo_local = i;
        e->relo_match.assign(match_points, match_points + (size_t)3 * n_match);
        std::memcpy(e->relo_prev, prev_relo_t, 24); std::memcpy(e->relo_prev + 3, prev_relo_r, 72);
        for (int c = 0; c < 3; c++) e->relo_pose[c] = e->Ps[i][c];      // the slot's pose as vector2double writes it (:1494-1503; the reference: see the header)
        R2q(e->Rs[i], e->relo_pose + 3);
        *accepted = 1;
        break;
    }
    return TCV_OK;
}
extern "C" int tcv_estimator_get_relocalization(const tcv_estimator *e, tcv_estimator_relo *out) {
    if (!e || !out) { tcv::set_error("estimator_get_relocalization: bad argument"); return TCV_ERR_INVALID; }
    *out = e->relo_out;
    return TCV_OK;
}

extern "C" int tcv_estimator_begin_frame(tcv_estimator *e, int n_imu, const double *acc, const double *gyr, int n_points, const int *point_ids,
                                         const double *points, int n_lines, const int *line_ids, const double *lines, const double *truth, int *ready) {
    if (!e || !ready || n_imu < 0 || n_points < 0 || n_lines < 0 || (n_points > 0 && (!point_ids || !points)) || (n_lines > 0 && !lines) ||
        (n_lines > 0 && e->assoc && !line_ids) || (n_imu > 0 && (!acc || !gyr))) { tcv::set_error("estimator_begin_frame: bad argument"); return TCV_ERR_INVALID; }
    if (e->phase != 0) { tcv::set_error("estimator_begin_frame: the previous frame has not been optimised and finished"); return TCV_ERR_INVALID; }
    // the tail of the front end's 7-vector staged for this frame (tcv_estimator_stage_point_aux): consumed here, used with ESTIMATE_TD only
    const int staged_n = e->staged_n;
    e->staged_n = -1;
    if (e->estimate_td && staged_n < 0) { tcv::set_error("estimator_begin_frame: estimate_td is on and no point aux (pixel position, velocity) was staged for this frame (tcv_estimator_stage_point_aux)"); return TCV_ERR_INVALID; }
    if (e->estimate_td && staged_n != n_points) { tcv::set_error("estimator_begin_frame: " + std::to_string(staged_n) + " points were staged with tcv_estimator_stage_point_aux, the frame has " + std::to_string(n_points)); return TCV_ERR_INVALID; }
    e->serials[e->frame_count] = e->next_serial++;      // (the frame's name for tcv_estimator_set_relo_frame: Headers[frame_count] = header)
    if (acc && gyr) process_imu(e, n_imu, acc, gyr);
    e->marg_flag = add_features_check_parallax(e, n_points, point_ids, points, e->estimate_td ? e->staged_aux.data() : nullptr, n_lines, line_ids, lines) ? MARGIN_OLD : MARGIN_SECOND_NEW;
    const int fc = e->frame_count;
    if (truth) { for (int c = 0; c < 3; c++) { e->Ps[fc][c] = truth[c]; e->Vs[fc][c] = truth[12 + c]; } std::memcpy(e->Rs[fc].data(), truth + 3, sizeof(double) * 9); }
    if (fc < W) {
        e->frame_count++;
        const int j = e->frame_count;
        e->Bas[j] = e->Bas[j - 1]; e->Bgs[j] = e->Bgs[j - 1]; e->Ps[j] = e->Ps[j - 1]; e->Rs[j] = e->Rs[j - 1]; e->Vs[j] = e->Vs[j - 1];
        *ready = 0;
        return TCV_OK;
    }
    *ready = 1;
    e->phase = 1;
    return TCV_OK;
}

extern "C" int tcv_estimators_begin_frames(tcv_estimator *const *es, int n, const tcv_frame_input *in, int *ready, int *rc_out) {
    if (!es || n <= 0 || !in || !ready) { tcv::set_error("estimators_begin_frames: bad argument"); return TCV_ERR_INVALID; }
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (es[i] == es[j]) { tcv::set_error("estimators_begin_frames: the same estimator twice"); return TCV_ERR_INVALID; }
    return first_failure(for_each_estimator_rc(n, [&](int i) {
        const tcv_frame_input &f = in[i];
        ready[i] = 0;
        return tcv_estimator_begin_frame(es[i], f.n_imu, f.acc, f.gyr, f.n_points, f.point_ids, f.points, f.n_lines, f.line_ids, f.lines, f.truth, &ready[i]);
    }), rc_out);
}

extern "C" int tcv_estimator_finish_frame(tcv_estimator *e, double P[3], double q[4], double V[3]) {
    if (!e || !P || !q || !V) return TCV_ERR_INVALID;
    if (e->phase != 2) { tcv::set_error("estimator_finish_frame: the window has not been optimised"); return TCV_ERR_INVALID; }
    e->phase = 0;
    if (e->opt_failed != TCV_OK) {      // the window's own solve / marginalisation failed in the lock-step batch: like failureDetection, the caller resets
        const int rc = e->opt_failed; e->opt_failed = TCV_OK;
        tcv::set_error("estimator: optimisation of this window failed: " + e->opt_msg);
        return rc;
    }
    if (failure_detection(e)) { tcv::set_error("failure detection (estimator.cpp:1629-1675): the estimator diverged"); return TCV_ERR_NUMERIC; }
    for (int c = 0; c < 3; c++) { P[c] = e->Ps[W][c]; V[c] = e->Vs[W][c]; }
    R2q(e->Rs[W], q);
    slide_window(e);
    e->last_P = e->Ps[W]; e->have_last = true;
    return TCV_OK;
}
extern "C" int tcv_estimators_finish_frames(tcv_estimator *const *es, int n, double *P, double *q, double *V, int *rc, tcv_estimator_stats *stats) {
    if (!es || n <= 0 || !P || !q || !V || !rc) return TCV_ERR_INVALID;
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (es[i] == es[j]) { tcv::set_error("estimators_finish_frames: the same estimator twice"); return TCV_ERR_INVALID; }
    return first_failure(for_each_estimator_rc(n, [&](int i) {
        if (stats && es[i]) stats[i] = es[i]->stats;
        return tcv_estimator_finish_frame(es[i], P + 3 * i, q + 4 * i, V + 3 * i);
    }), rc);
}
extern "C" int tcv_estimator_set_window_tap(tcv_estimator *e, int on) {
    if (!e) return TCV_ERR_INVALID;
    e->tap.on = on != 0;
    if (!on) e->tap = WindowTap();
    return TCV_OK;
}
extern "C" int tcv_estimator_get_stats(const tcv_estimator *e, tcv_estimator_stats *out) {
    if (!e || !out) return TCV_ERR_INVALID;
    *out = e->stats;
    return TCV_OK;
}
