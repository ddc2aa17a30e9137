// Native estimator, internal: its host math, its tracks, the state of one estimator in parts, and what its four files share
// (tcv_est_tracks.cpp: the device-free bookkeeping; tcv_est_window.cpp: one estimator's calls into the library; tcv_est_lockstep.cpp: the
// lock-step frame; tcv_estimator.cpp: the C-ABI of one estimator).  Nothing of HIP in here: tcv_est_tracks.cpp compiles with a plain host compiler.
#pragma once
#include <array>
#include <cmath>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tcv_estimator.h"

struct EstInflight;      // (tcv_est_lockstep.cpp) a lock-step frame whose marginalisation is still to be launched or asked about

namespace tcv_est {

constexpr int W = 10;                      // WINDOW_SIZE (parameters.h:20)
enum { MARGIN_OLD = 0, MARGIN_SECOND_NEW = 1 };
typedef std::array<double, 3> V3;
typedef std::array<double, 9> M3;          // row-major

inline V3 add(const V3 &a, const V3 &b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline V3 sub(const V3 &a, const V3 &b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline V3 scl(const V3 &a, double s) { return {a[0] * s, a[1] * s, a[2] * s}; }
inline double nrm(const V3 &a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
inline V3 mv(const M3 &m, const V3 &v) { return {m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[3] * v[0] + m[4] * v[1] + m[5] * v[2], m[6] * v[0] + m[7] * v[1] + m[8] * v[2]}; }
inline M3 mm(const M3 &a, const M3 &b) {
    M3 c;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
    return c;
}
inline M3 tr(const M3 &a) { return {a[0], a[3], a[6], a[1], a[4], a[7], a[2], a[5], a[8]}; }
inline M3 eye() { return {1, 0, 0, 0, 1, 0, 0, 0, 1}; }
// Eigen toRotationMatrix of q = (x y z w), no normalisation
inline M3 q2R(const double q[4]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    return {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
}
// Eigen `Quaterniond q{R}` (vector2double, estimator.cpp:1499), x y z w
inline void R2q(const M3 &m, double q[4]) {
    auto M = [&](int r, int c) { return m[3 * r + c]; };
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0) {
        t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (M(2, 1) - M(1, 2)) * t; q[1] = (M(0, 2) - M(2, 0)) * t; q[2] = (M(1, 0) - M(0, 1)) * t;
    } else {
        int i = 0;
        if (M(1, 1) > M(0, 0)) i = 1;
        if (M(2, 2) > M(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (M(k, j) - M(j, k)) * t; q[j] = (M(j, i) + M(i, j)) * t; q[k] = (M(k, i) + M(i, k)) * t;
    }
}
// Utility::deltaQ(theta).toRotationMatrix() (utility.h:15-28; not normalised, like the reference)
inline M3 deltaQ_R(const V3 &th) { const double q[4] = {th[0] / 2, th[1] / 2, th[2] / 2, 1.0}; return q2R(q); }

struct Feature {
    int id, start;
    std::vector<V3> obs;
    std::vector<std::array<double, 5>> aux;      // ESTIMATE_TD only, one per observation: uv (pixels), velocity (normalised plane), cur_td (feature_manager.h:138-149); empty otherwise
    double depth = -1.0;       // FeaturePerId ctor: estimated_depth(-1.0)
    int solve_flag = 0;
    int end() const { return start + (int)obs.size() - 1; }
};
struct LineObs {
    double vec[4], abc[3], world[6];
    double errA = -1, errD = -1, overlap = -1;
    bool credible_line = true, use_flag = false;
};
struct LineFeature { int id, start; std::vector<LineObs> obs; bool credible_matching = true; };
struct GivenLine { double d[9]; };          // 3D start, 3D end (world), A B C
struct ImuBuf {
    bool valid = false;
    V3 acc0, gyr0, ba, bg;
    std::vector<V3> acc, gyr;
};

// The factor lists of one problem: the window's, its marginalisation problem's, and the tap's copy of the window's.
struct FactorLists {
    std::vector<tcv_imu_preintegration> imu;
    std::vector<const tcv_preint *> imu_dev;      // the same factors as device-resident handles (empty: host pre-integrations; entries may be null: that factor's host copy is used)
    std::vector<int> imu_i, imu_j;
    std::vector<int> pi, pj, pl;                  // projection factors: frame i, frame j, landmark
    std::vector<double> pts, aux;                 // n_proj x 6 (pts_i | pts_j); proj_td_aux, n_proj x 8 (ESTIMATE_TD only)
    std::vector<int> lf;                          // line factors: frame
    std::vector<double> ld;                       // n_line x 9
    void clear() { imu.clear(); imu_dev.clear(); imu_i.clear(); imu_j.clear(); pi.clear(); pj.clear(); pl.clear(); pts.clear(); aux.clear(); lf.clear(); ld.clear(); }      // (keeps the capacity)
    // counts and arrays, under the names tcv_window_desc and tcv_window_snapshot share
    template <class D> void bind_lists(D &d) const {
        d.n_imu = (int)imu.size(); d.imu = imu.data(); d.imu_frame_i = imu_i.data(); d.imu_frame_j = imu_j.data();
        d.n_proj = (int)pi.size(); d.proj_frame_i = pi.data(); d.proj_frame_j = pj.data(); d.proj_feature = pl.data(); d.proj_pts = pts.data();
        d.n_line = (int)lf.size(); d.line_frame = lf.data(); d.line_data = ld.data();
    }
    void bind(tcv_window_desc &d, bool with_td) const {
        bind_lists(d);
        d.imu_device = imu_dev.empty() ? nullptr : imu_dev.data();
        if (with_td) d.proj_td_aux = aux.data();
    }
};

// snapshot of the window an estimator handed to the solver (tcv_estimator_set_window_tap)
struct WindowTap {
    bool on = false, have = false;
    std::vector<double> pose_in, sb_in, ex_in, feat_in, pose_out, sb_out, ex_out, feat_out, x0, J0, r0;
    FactorLists f;             // (device-resident pre-integrations materialised, imu_dev empty)
    double td_in = 0, td_out = 0;
    // relocalisation part (tcv_window_snapshot_relo)
    bool has_relo = false;
    int relo_local = 0, relo_frame_index = 0, relo_frame_serial = 0;
    double relo_in[7], relo_out[7], relo_prev[12];
    std::vector<int> r_pi, r_pl;
    std::vector<double> r_pts;
    tcv_relo_result relo_result;
    std::vector<int> pk, pidx, psize, pcol;
    double Ric[9];
    int marg_flag = 0, prior_m = 0, prior_n = 0, iterations = 0, applied = 0;
    double final_cost = 0;
};

// ---- the state of one estimator, in parts.  Every part but the settings is given a fresh value by tcv_estimator_reset. ----
struct EstSettings {
    tcv_estimator_config cfg;
    bool assoc = false;                      // the line map (tcv_estimator_set_line_map)
    std::vector<double> map_lines;           // n x 6
    std::shared_ptr<tcv_line_map> map_dev;   // the same lines resident on the device (created with set_line_map; null: uploaded per call)
    int n_map = 0;
    M3 Rbw;
    V3 Tbw;
    // ESTIMATE_TD (tcv_estimator_set_time_offset): the globals ESTIMATE_TD / TD / TR / ROW (parameters.cpp:135-138)
    int estimate_td = 0;
    double td0 = 0.0, td_TR = 0.0, td_ROW = 1.0;
};
struct EstStates {
    V3 Ps[W + 1] = {}, Vs[W + 1] = {}, Bas[W + 1] = {}, Bgs[W + 1] = {};
    M3 Rs[W + 1];
    V3 tic = {};                             // (reset: the configured extrinsic)
    M3 ric = {};
    int frame_count = 0, marg_flag = MARGIN_OLD;
    int next_serial = 0;                     // frame serials stand in for Headers[i].stamp (tcv_estimator_relo.h)
    int serials[W + 1];                      // serial of the frame in every slot, -1: none
    bool have_acc0 = false, have_last = false;
    V3 acc_0 = {}, gyr_0 = {}, last_P = {};
    EstStates() { for (int i = 0; i <= W; i++) { Rs[i] = eye(); serials[i] = -1; } }
};
struct EstImu {
    ImuBuf bufs[W + 1];
    tcv_imu_preintegration pre[W + 1] = {};  // host copy (TCV_EST_HOST_PREINT=1), otherwise only sum_dt is filled in
    std::shared_ptr<tcv_preint> preh[W + 1]; // pre_integrations[] on the device (estimator.h: pre_integrations[WINDOW_SIZE + 1]); slots share a handle while a slide copies them
    bool pre_valid[W + 1] = {};
};
struct EstTracks {
    std::vector<Feature> features;
    std::vector<LineFeature> linefeatures;
    std::vector<GivenLine> line_obs[W + 1];
    std::vector<unsigned char> fov[W + 1];   // WorldLinesInFOV[i] as a mask over the map (empty: not set)
    bool fov_ready = false;
};
// the window handed to the solver (parameter blocks are identified by address: the arrays live, in place, as long as the estimator)
struct EstWindow {
    double para_pose[(W + 1) * 7] = {}, para_sb[(W + 1) * 9] = {}, para_ex[7] = {};
    std::vector<double> para_feature;
    std::vector<int> sel;                    // indices into `features` of the landmarks of the current window
    FactorLists w, m;                        // the current window's factors; its marginalisation problem's (never line factors; MARGIN_SECOND_NEW: none at all)
    std::vector<double *> m_drop;
    double w_Ric[9] = {};
    std::vector<int> w_pk, w_pidx;
    int n_line_obs_total = 0;
};
struct EstPriorChain {
    tcv_prior *prior = nullptr;              // (owned: released before the part is reset)
    std::vector<std::pair<int, int>> prior_blocks;      // (kind 0 pose / 1 sb / 2 ex / 3 td, index)
    std::shared_ptr<EstInflight> prev;       // the frame whose marginalisation produced `prior` and may still be running; prev_k: this estimator's window in it
    int prev_k = -1;
    std::shared_ptr<EstInflight> pend;       // the frame whose marginalisation has not been launched yet (EstInflight::launch): its prior is taken at the start of the next tcv_estimators_optimize
    int pend_k = -1, pend_flag = MARGIN_OLD;
    int pend_failed = 0;                     // != TCV_OK: the previous frame's (deferred) marginalisation could not be launched: this frame's window is solved without
    std::string pend_msg;                    // its prior, nothing of it is applied and finish_frame reports the failure (the caller resets, like after failureDetection)
};
struct EstTd {      // Estimator::td and para_Td[0] (reset: td0)
    double td = 0.0;
    double para_td[1] = {0.0};
    std::vector<double> staged_aux;          // tcv_estimator_stage_point_aux: n x 4 for the next begin_frame
    int staged_n = -1;                       // -1: nothing staged
};
// relocalisation (tcv_estimator_relo.h): the request of setReloFrame (estimator.cpp:2261-2279) waits for the next optimised window, whose
// relo_Pose block and factors (:1854-1886) are the r_* lists; relo_out is what the last applied relocalisation window left (:1606-1620)
struct EstRelo {
    bool relo_pending = false;
    int relo_serial = -1, relo_frame_index = 0, relo_local = -1;
    std::vector<double> relo_match;          // n x 3: x, y, feature id (ascending)
    double relo_prev[12] = {};               // prev_relo_t | prev_relo_r
    double relo_pose[7] = {0, 0, 0, 0, 0, 0, 1};      // relo_Pose: a parameter block of the window (identified by address)
    bool w_relo = false;                     // the current window carries it
    int w_relo_local = -1, w_relo_frame_index = 0, w_relo_serial = -1;
    double w_relo_prev[12] = {};
    std::vector<int> r_pi, r_pl;             // start_frame and feature_index of every relocalisation factor
    std::vector<double> r_pts;               // pts_i | pts_j
    tcv_estimator_relo relo_out = {};        // relocalization_info = 0, drift_correct_r = Identity, drift_correct_t = Zero (estimator.cpp:185-188)
    EstRelo() { relo_out.drift_correct_r[0] = relo_out.drift_correct_r[4] = relo_out.drift_correct_r[8] = 1.0; }
};
struct EstFrame {
    int phase = 0;                           // 0: between frames, 1: window full, waiting for the optimisation, 2: optimised, waiting for finish_frame
    int opt_failed = 0;                      // != TCV_OK: this estimator's window failed in the last lock-step batch (reported by finish_frame)
    std::string opt_msg;
    tcv_estimator_stats stats = {};
};

}  // namespace tcv_est

// What survives tcv_estimator_reset: EstSettings and the tap, nothing else.  The configuration and the line map stay because the reference's
// clearState() + setParameter() keep them (the map is loaded once, setParameters, estimator.cpp:54-124); the td settings and the tap are
// this library's own choice: both are set once per estimator, like the configuration, and a caller that resets after a failure goes on
// with them.  Every other part is a value that reset() replaces by a fresh one, so a field added to it is reset by default.  The parts are
// bases, not members, so that the parameter blocks (para_pose, para_sb, para_ex, para_td, relo_pose) keep their address for the life of
// the estimator -- an assignment writes them in place -- and the code reads e->Ps as it always did.
struct tcv_estimator : tcv_est::EstSettings, tcv_est::EstStates, tcv_est::EstImu, tcv_est::EstTracks, tcv_est::EstWindow, tcv_est::EstPriorChain, tcv_est::EstTd,
                       tcv_est::EstRelo, tcv_est::EstFrame {
    tcv_est::WindowTap tap;
    template <class Part> void fresh() { static_cast<Part &>(*this) = Part(); }
};

namespace tcv_est {

// ---- tcv_est_tracks.cpp: the mirror of feature_manager.cpp and of the slide.  No device, no call into the library. ----
void process_imu(tcv_estimator *e, int n, const double *acc, const double *gyr);
bool add_features_check_parallax(tcv_estimator *e, int n_points, const int *ids, const double *pts, const double *aux4, int n_lines, const int *line_ids, const double *lines);
void triangulate(tcv_estimator *e);
void poses_of(const tcv_estimator *e, double pose[(W + 1) * 7], double ex[7]);
void remove_line_outlier(tcv_estimator *e);
int build_window(tcv_estimator *e);
void build_marg(tcv_estimator *e, int flag);
void apply_states(tcv_estimator *e);
bool failure_detection(const tcv_estimator *e);
void slide_window(tcv_estimator *e);

// ---- tcv_est_window.cpp: what one estimator asks of the library ----
// The 2D-3D association of one estimator, in two halves around the device call so that the estimators of a lock-step frame share ONE
// tcv_match_lines_batch (one upload, one download, one wait for all of them instead of a round trip each).
struct AssocJob {
    double pose[(W + 1) * 7], ex[7];
    std::vector<int> det_frame, match;
    std::vector<double> det;
    std::vector<LineObs *> where;
    std::vector<unsigned char> given;
    std::vector<float> err;
    bool one_call = false, call = false;
    tcv_match_lines_args args;
};
int assoc_prepare(tcv_estimator *e, AssocJob &J);
void assoc_finish(tcv_estimator *e, AssocJob &J);
void fill_desc(tcv_estimator *e, tcv_window_desc &d, bool marg);
int take_prior(tcv_estimator *e, tcv_prior *np, int flag);
int tap_window(tcv_estimator *e);

// ---- tcv_est_lockstep.cpp: per-estimator host work on the library's worker threads ----
struct TaskRc { int rc = TCV_OK; std::string msg; };
std::vector<TaskRc> for_each_estimator_rc(int n, const std::function<int(int)> &fn, bool on_caller = false);
int first_failure(const std::vector<TaskRc> &r, int *rcs_out = nullptr);

}  // namespace tcv_est
