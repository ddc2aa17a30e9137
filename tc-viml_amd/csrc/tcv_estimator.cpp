// Native mirror of the estimator's per-frame window management around the hot path (include/tcv_estimator.h).
// Reference: vins_estimator/src/estimator.cpp (processIMU :191-228, processImagewithLine :230-383, solveOdometry :1476-1490,
// double2vector :1537-1627, failureDetection :1629-1675, slideWindowWithLinesFoV :2121-2259, prior chaining :2027-2044 / :2083-2113)
// and feature_manager.cpp (addFeaturesCheckParallax :260-334, setDepth :379-397, removeFailures :399-408, triangulate :440-492,
// removeLineOutlier :494-534, removeBackShiftDepth :559-616, removeFront :655-696, compensatedParallax2 :698-734).
// Host code only: every numerical step of the hot path goes through the C-ABI of tcv.h (HIP kernels); there is no CPU solver here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tcv_estimator.h"
#include "tcv_hostpool.h"      // parallel_items, async_run, HostOp: the persistent host worker threads
#include "tcv_runtime.h"       // util_stream, aux_stream, set_error

int tcv_marg_layout_n(const tcv_batch *b, int window);      // (tcv_marg_host.cpp: n of the prior a window's attached marginalisation problem makes, known before the kernel runs)

namespace {

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

// smallest right singular vector of A (rows x 4): one-sided Jacobi on the columns (what JacobiSVD in triangulate() delivers)
void smallest_right_singular_vector(std::vector<std::array<double, 4>> A, double v_out[4]) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    const int m = (int)A.size();
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double a = 0, b = 0, c = 0;
                for (int i = 0; i < m; i++) { a += A[i][p] * A[i][p]; b += A[i][q] * A[i][q]; c += A[i][p] * A[i][q]; }
                if (std::fabs(c) <= 1e-300 || std::fabs(c) <= 2.3e-16 * std::sqrt(a * b)) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < m; i++) { const double x = A[i][p], y = A[i][q]; A[i][p] = cs * x - sn * y; A[i][q] = sn * x + cs * y; }
                for (int i = 0; i < 4; i++) { const double x = V[i][p], y = V[i][q]; V[i][p] = cs * x - sn * y; V[i][q] = sn * x + cs * y; }
            }
        if (!rotated) break;
    }
    int best = 0;
    double bn = -1;
    for (int j = 0; j < 4; j++) {
        double s = 0;
        for (int i = 0; i < m; i++) s += A[i][j] * A[i][j];
        if (bn < 0 || s < bn) { bn = s; best = j; }
    }
    for (int i = 0; i < 4; i++) v_out[i] = V[i][best];
}

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

}  // namespace

// kernel-time accounting of the lock-step frames (tcv_estimators_kernel_profile): HIP-event durations of the solve and marginalisation
// launches, the windows they held and those windows' ALGORITHMIC bytes x linearisations -- what bench.py --mode replay
// prices against the HBM roofline
std::mutex g_kmu;
double g_kern[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // solve ms, solve launches, marginalisation ms, marginalisation launches, windows, bytes x linearisations, linearisations, marginalised windows
void kern_add(int slot, double v) { std::lock_guard<std::mutex> g(g_kmu); g_kern[slot] += v; }

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

// snapshot of the window an estimator handed to the solver (tcv_estimator_set_window_tap)
struct WindowTap {
    bool on = false, have = false;
    std::vector<double> pose_in, sb_in, ex_in, feat_in, pose_out, sb_out, ex_out, feat_out, pts, ld, x0, J0, r0, aux;
    double td_in = 0, td_out = 0;
    // relocalisation part (tcv_window_snapshot_relo)
    bool has_relo = false;
    int relo_local = 0, relo_frame_index = 0, relo_frame_serial = 0;
    double relo_in[7], relo_out[7], relo_prev[12];
    std::vector<int> r_pi, r_pl;
    std::vector<double> r_pts;
    tcv_relo_result relo_result;
    std::vector<tcv_imu_preintegration> imu;
    std::vector<int> imu_i, imu_j, pi, pj, pl, lf, pk, pidx, psize, pcol;
    double Ric[9];
    int marg_flag = 0, prior_m = 0, prior_n = 0, iterations = 0, applied = 0;
    double final_cost = 0;
};

struct tcv_estimator {
    tcv_estimator_config cfg;
    WindowTap tap;
    std::shared_ptr<EstInflight> prev;       // the frame whose marginalisation produced `prior` and may still be running; prev_k: this estimator's window in it
    int prev_k = -1;
    std::shared_ptr<EstInflight> pend;       // the frame whose marginalisation has not been launched yet (EstInflight::launch): its prior is taken at the start of the next tcv_estimators_optimize
    int pend_k = -1, pend_flag = MARGIN_OLD;
    V3 Ps[W + 1], Vs[W + 1], Bas[W + 1], Bgs[W + 1];
    M3 Rs[W + 1];
    V3 tic;
    M3 ric;
    ImuBuf bufs[W + 1];
    tcv_imu_preintegration pre[W + 1];       // host copy (TCV_EST_HOST_PREINT=1), otherwise only sum_dt is filled in
    std::shared_ptr<tcv_preint> preh[W + 1]; // pre_integrations[] on the device (estimator.h: pre_integrations[WINDOW_SIZE + 1]); slots share a handle while a slide copies them
    bool pre_valid[W + 1];
    std::vector<Feature> features;
    std::vector<GivenLine> line_obs[W + 1];
    bool assoc = false;
    std::vector<double> map_lines;           // n x 6
    std::shared_ptr<tcv_line_map> map_dev;   // the same lines resident on the device (created with set_line_map; null: uploaded per call)
    int n_map = 0;
    M3 Rbw;
    V3 Tbw;
    std::vector<LineFeature> linefeatures;
    std::vector<unsigned char> fov[W + 1];   // WorldLinesInFOV[i] as a mask over the map (empty: not set)
    bool fov_ready = false;
    tcv_prior *prior = nullptr;
    std::vector<std::pair<int, int>> prior_blocks;      // (kind 0 pose / 1 sb / 2 ex / 3 td, index)
    int frame_count = 0, marg_flag = MARGIN_OLD;
    bool have_acc0 = false, have_last = false;
    V3 acc_0, gyr_0, last_P;
    tcv_estimator_stats stats;
    // the window handed to the solver (parameter blocks are identified by address: these arrays live as long as the estimator)
    double para_pose[(W + 1) * 7], para_sb[(W + 1) * 9], para_ex[7];
    std::vector<double> para_feature;
    std::vector<int> sel;                    // indices into `features` of the landmarks of the current window
    // factor lists of the current window
    std::vector<tcv_imu_preintegration> w_imu;
    std::vector<const tcv_preint *> w_imu_dev, m_imu_dev;      // the same factors as device-resident handles (empty: host pre-integrations)
    std::vector<int> w_imu_i, w_imu_j, w_pi, w_pj, w_pl, w_lf;
    std::vector<double> w_pts, w_ld;
    double w_Ric[9];
    std::vector<int> w_pk, w_pidx;
    // marginalisation sub-problem
    std::vector<tcv_imu_preintegration> m_imu;
    std::vector<int> m_imu_i, m_imu_j, m_pi, m_pj, m_pl;
    std::vector<double> m_pts;
    std::vector<double *> m_drop;
    int n_line_obs_total = 0;
    int phase = 0;                           // 0: between frames, 1: window full, waiting for the optimisation, 2: optimised, waiting for finish_frame
    int opt_failed = 0;                      // != TCV_OK: this estimator's window failed in the last lock-step batch (reported by finish_frame)
    std::string opt_msg;
    // ESTIMATE_TD (tcv_estimator_set_time_offset): the globals ESTIMATE_TD / TD / TR / ROW (parameters.cpp:135-138), Estimator::td and para_Td[0]
    int estimate_td = 0;
    double td0 = 0.0, td = 0.0, td_TR = 0.0, td_ROW = 1.0;
    double para_td[1] = {0.0};
    std::vector<double> staged_aux;          // tcv_estimator_stage_point_aux: n x 4 for the next begin_frame
    int staged_n = -1;                       // -1: nothing staged
    std::vector<double> w_aux, m_aux;        // proj_td_aux of the window / of its marginalisation problem (n_proj x 8)
    // relocalisation (tcv_estimator_relo.h).  Frame serials stand in for Headers[i].stamp; the request of setReloFrame (estimator.cpp:2261-2279)
    // waits for the next optimised window, whose relo_Pose block and factors (:1854-1886) are the r_* lists; relo_out is what the last
    // applied relocalisation window left (:1606-1620)
    int next_serial = 0;
    int serials[W + 1];                      // serial of the frame in every slot, -1: none
    bool relo_pending = false;
    int relo_serial = -1, relo_frame_index = 0, relo_local = -1;
    std::vector<double> relo_match;          // n x 3: x, y, feature id (ascending)
    double relo_prev[12];                    // prev_relo_t | prev_relo_r
    double relo_pose[7] = {0, 0, 0, 0, 0, 0, 1};      // relo_Pose: a parameter block of the window (identified by address)
    bool w_relo = false;                     // the current window carries it
    int w_relo_local = -1, w_relo_frame_index = 0, w_relo_serial = -1;
    double w_relo_prev[12];
    std::vector<int> r_pi, r_pl;             // start_frame and feature_index of every relocalisation factor
    std::vector<double> r_pts;               // pts_i | pts_j
    tcv_estimator_relo relo_out;
    int pend_failed = 0;                     // != TCV_OK: the previous frame's (deferred) marginalisation could not be launched: this frame's window is solved without
    std::string pend_msg;                    // its prior, nothing of it is applied and finish_frame reports the failure (the caller resets, like after failureDetection)
};
// the device-resident line map is bound to the device that was current at tcv_estimator_set_line_map: an estimator optimised with another
// current device uses the host copy it still holds (uploaded with the call) instead of failing the association (round-5 advisor finding)
extern "C" int tcv_line_map_device(const tcv_line_map *m);
static inline const tcv_line_map *map_on_current_device(const tcv_estimator *e) {
    if (!e->map_dev) return nullptr;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    return tcv_line_map_device(e->map_dev.get()) == cur ? e->map_dev.get() : nullptr;
}

namespace {

void process_imu(tcv_estimator *e, int n, const double *acc, const double *gyr) {
    const int j = e->frame_count;
    auto row = [](const double *a, int i) { return V3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; };
    if (!e->have_acc0) { e->acc_0 = row(acc, 0); e->gyr_0 = row(gyr, 0); e->have_acc0 = true; }
    ImuBuf &b = e->bufs[j];
    if (!b.valid) { b.valid = true; b.acc0 = e->acc_0; b.gyr0 = e->gyr_0; b.ba = e->Bas[j]; b.bg = e->Bgs[j]; b.acc.clear(); b.gyr.clear(); }
    const double dt = e->cfg.imu_dt;
    const V3 G = {e->cfg.gravity[0], e->cfg.gravity[1], e->cfg.gravity[2]};
    for (int i = 1; i <= n; i++) {
        const V3 a = row(acc, i), w = row(gyr, i);
        if (j != 0) {
            b.acc.push_back(a); b.gyr.push_back(w);
            const V3 un_acc_0 = sub(mv(e->Rs[j], sub(e->acc_0, e->Bas[j])), G);            // estimator.cpp:217-224
            const V3 un_gyr = sub(scl(add(e->gyr_0, w), 0.5), e->Bgs[j]);
            e->Rs[j] = mm(e->Rs[j], deltaQ_R(scl(un_gyr, dt)));
            const V3 un_acc_1 = sub(mv(e->Rs[j], sub(a, e->Bas[j])), G);
            const V3 un_acc = scl(add(un_acc_0, un_acc_1), 0.5);
            e->Ps[j] = add(add(e->Ps[j], scl(e->Vs[j], dt)), scl(un_acc, 0.5 * dt * dt));
            e->Vs[j] = add(e->Vs[j], scl(un_acc, dt));
        }
        e->acc_0 = a; e->gyr_0 = w;
    }
    e->pre_valid[j] = false;
}

bool add_features_check_parallax(tcv_estimator *e, int n_points, const int *ids, const double *pts, const double *aux4, int n_lines, const int *line_ids, const double *lines) {
    const int fc = e->frame_count;
    std::unordered_map<int, int> by_id;
    for (size_t k = 0; k < e->features.size(); k++) by_id[e->features[k].id] = (int)k;
    int last_track_num = 0;
    for (int k = 0; k < n_points; k++) {
        auto it = by_id.find(ids[k]);
        int idx;
        if (it == by_id.end()) {
            Feature f; f.id = ids[k]; f.start = fc;
            e->features.push_back(f); idx = (int)e->features.size() - 1; by_id[ids[k]] = idx;
        } else { idx = it->second; last_track_num++; }
        e->features[idx].obs.push_back(V3{pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]});
        if (aux4) e->features[idx].aux.push_back({aux4[4 * k], aux4[4 * k + 1], aux4[4 * k + 2], aux4[4 * k + 3], e->td});      // FeaturePerFrame(point, td) (feature_manager.cpp:215, :271)
    }
    if (e->assoc) {      // the line tracker's (id, end points): addFeaturesCheckParallax :291-311
        std::unordered_map<int, int> by_lid;
        for (size_t k = 0; k < e->linefeatures.size(); k++) by_lid[e->linefeatures[k].id] = (int)k;
        for (int k = 0; k < n_lines; k++) {
            auto it = by_lid.find(line_ids[k]);
            int idx;
            if (it == by_lid.end()) {
                LineFeature lf; lf.id = line_ids[k]; lf.start = fc;
                e->linefeatures.push_back(lf); idx = (int)e->linefeatures.size() - 1; by_lid[line_ids[k]] = idx;
            } else idx = it->second;
            LineObs ob;
            const double *v = lines + 4 * k;
            for (int i = 0; i < 4; i++) ob.vec[i] = v[i];
            ob.abc[0] = v[3] - v[1]; ob.abc[1] = v[0] - v[2]; ob.abc[2] = v[2] * v[1] - v[0] * v[3];      // feature_manager.cpp:11-13
            for (int i = 0; i < 6; i++) ob.world[i] = 0.0;
            e->linefeatures[idx].obs.push_back(ob);
        }
    } else {
        e->line_obs[fc].clear();
        for (int k = 0; k < n_lines; k++) { GivenLine g; std::memcpy(g.d, lines + 9 * k, sizeof g.d); e->line_obs[fc].push_back(g); }
    }
    if (fc < 2 || last_track_num < 20) return true;
    double s = 0;
    int n = 0;
    for (auto &f : e->features)
        if (f.start <= fc - 2 && f.end() >= fc - 1) {
            const V3 &pi = f.obs[fc - 2 - f.start], &pj = f.obs[fc - 1 - f.start];      // compensatedParallax2 (:698-734)
            const double du = pi[0] / pi[2] - pj[0], dv = pi[1] / pi[2] - pj[1];
            s += std::sqrt(du * du + dv * dv); n++;
        }
    return n == 0 ? true : (s / n >= e->cfg.min_parallax);
}

bool selected(const Feature &f) { return f.obs.size() >= 2 && f.start < W - 2; }

void triangulate(tcv_estimator *e) {
    for (auto &f : e->features) {
        if (!selected(f) || f.depth > 0) continue;
        const int i = f.start;
        const V3 t0 = add(e->Ps[i], mv(e->Rs[i], e->tic));
        const M3 R0 = mm(e->Rs[i], e->ric);
        std::vector<std::array<double, 4>> A;
        for (size_t k = 0; k < f.obs.size(); k++) {
            const int j = i + (int)k;
            const V3 t1 = add(e->Ps[j], mv(e->Rs[j], e->tic));
            const M3 R1 = mm(e->Rs[j], e->ric);
            const V3 t = mv(tr(R0), sub(t1, t0));
            const M3 R = mm(tr(R0), R1), Rt = tr(R);
            const V3 mt = scl(mv(Rt, t), -1.0);
            double P[3][4];
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) P[r][c] = Rt[3 * r + c]; P[r][3] = mt[r]; }
            const V3 fn = scl(f.obs[k], 1.0 / nrm(f.obs[k]));
            std::array<double, 4> r0, r1;
            for (int c = 0; c < 4; c++) { r0[c] = fn[0] * P[2][c] - fn[2] * P[0][c]; r1[c] = fn[1] * P[2][c] - fn[2] * P[1][c]; }
            A.push_back(r0); A.push_back(r1);
        }
        double v[4];
        smallest_right_singular_vector(A, v);
        f.depth = v[2] / v[3];
        if (f.depth < 0.1) f.depth = e->cfg.init_depth;
    }
}

void poses_of(const tcv_estimator *e, double pose[(W + 1) * 7], double ex[7]) {
    for (int i = 0; i <= W; i++) { for (int c = 0; c < 3; c++) pose[7 * i + c] = e->Ps[i][c]; R2q(e->Rs[i], pose + 7 * i + 3); }
    for (int c = 0; c < 3; c++) ex[c] = e->tic[c];
    R2q(e->ric, ex + 3);
}

// UpdateLinesInFoV / initialLineFoVWindow, updateLinePairInWindow and removeLineOutlier, as processImagewithLine runs them before
// solveOdometry (estimator.cpp:328-336, :385-497; feature_manager.cpp:494-534)
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
    if (nd > 0) {
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
    }
    for (auto &lf : e->linefeatures) {                    // removeLineOutlier
        if (lf.obs.empty()) continue;
        const double *first = lf.obs[0].world;
        int count = 0;
        for (auto &ob : lf.obs) {
            double d2 = 0;
            for (int c = 0; c < 3; c++) { const double d = (ob.world[3 + c] - ob.world[c]) - (first[3 + c] - first[c]); d2 += d * d; }
            ob.credible_line = !((float)std::sqrt(d2) > 0.1f);
            count += ob.credible_line ? 0 : 1;
        }
        lf.credible_matching = !((count / (int)lf.obs.size()) >= 0.5);
    }
}

// vector2double (estimator.cpp:1492-1535) + the factor lists OptimizationWithLine walks (:1683-1846)
int build_window(tcv_estimator *e) {
    poses_of(e, e->para_pose, e->para_ex);
    for (int i = 0; i <= W; i++) for (int c = 0; c < 3; c++) { e->para_sb[9 * i + c] = e->Vs[i][c]; e->para_sb[9 * i + 3 + c] = e->Bas[i][c]; e->para_sb[9 * i + 6 + c] = e->Bgs[i][c]; }
    e->sel.clear();
    for (size_t k = 0; k < e->features.size(); k++) if (selected(e->features[k])) e->sel.push_back((int)k);
    e->para_feature.resize(std::max<size_t>(1, e->sel.size()));
    for (size_t l = 0; l < e->sel.size(); l++) e->para_feature[l] = 1.0 / e->features[e->sel[l]].depth;
    if (e->estimate_td) e->para_td[0] = e->td;      // :1533-1534
    e->w_imu.clear(); e->w_imu_i.clear(); e->w_imu_j.clear(); e->w_imu_dev.clear();
    for (int k = 0; k < W; k++)
        if (e->pre[k + 1].sum_dt <= 10.0) {      // estimator.cpp:1726
            e->w_imu.push_back(e->pre[k + 1]); e->w_imu_i.push_back(k); e->w_imu_j.push_back(k + 1);
            e->w_imu_dev.push_back(e->preh[k + 1].get());
        }
    e->w_pi.clear(); e->w_pj.clear(); e->w_pl.clear(); e->w_pts.clear(); e->w_aux.clear();
    for (size_t l = 0; l < e->sel.size(); l++) {      // estimator.cpp:1737-1771
        const Feature &f = e->features[e->sel[l]];
        for (size_t k = 1; k < f.obs.size(); k++) {
            e->w_pi.push_back(f.start); e->w_pj.push_back(f.start + (int)k); e->w_pl.push_back((int)l);
            e->w_pts.insert(e->w_pts.end(), f.obs[0].begin(), f.obs[0].end()); e->w_pts.insert(e->w_pts.end(), f.obs[k].begin(), f.obs[k].end());
            if (e->estimate_td) {      // the constructor arguments of ProjectionTdFactor (:1757-1763): velocities, cur_td, uv.y() of the anchor and of observation k
                const std::array<double, 5> &a = f.aux[0], &b = f.aux[k];
                const double x[8] = {a[2], a[3], b[2], b[3], a[4], b[4], a[1], b[1]};
                e->w_aux.insert(e->w_aux.end(), x, x + 8);
            }
        }
    }
    // relocalisation (:1854-1886): relo_Pose and one ProjectionFactor per matched feature that starts at or before the matched frame.  The
    // match list is walked once, in the order of the feature list, like :1870-1874 -- with an end check the reference does not have
    e->w_relo = false; e->r_pi.clear(); e->r_pl.clear(); e->r_pts.clear();
    if (e->relo_pending) {
        e->relo_pending = false;      // this window consumes the request, applied or not
        const size_t nm = e->relo_match.size() / 3;
        size_t r = 0;
        for (size_t l = 0; l < e->sel.size(); l++) {
            const Feature &f = e->features[e->sel[l]];
            if (f.start > e->relo_local) continue;
            while (r < nm && (int)e->relo_match[3 * r + 2] < f.id) r++;
            if (r < nm && (int)e->relo_match[3 * r + 2] == f.id) {
                e->r_pi.push_back(f.start); e->r_pl.push_back((int)l);
                e->r_pts.insert(e->r_pts.end(), f.obs[0].begin(), f.obs[0].end());
                const double pj[3] = {e->relo_match[3 * r], e->relo_match[3 * r + 1], 1.0};
                e->r_pts.insert(e->r_pts.end(), pj, pj + 3);
                r++;
            }
        }
        if (!e->r_pi.empty()) {
            e->w_relo = true; e->w_relo_local = e->relo_local; e->w_relo_frame_index = e->relo_frame_index; e->w_relo_serial = e->relo_serial;
            std::memcpy(e->w_relo_prev, e->relo_prev, sizeof e->w_relo_prev);
        }
    }
    e->w_lf.clear(); e->w_ld.clear();
    e->n_line_obs_total = 0;
    if (!e->assoc) {
        for (int i = 0; i <= W; i++) for (auto &g : e->line_obs[i]) { e->w_lf.push_back(i); e->w_ld.insert(e->w_ld.end(), g.d, g.d + 9); }
    } else {      // estimator.cpp:1786-1846
        for (auto &lf : e->linefeatures) {
            e->n_line_obs_total += (int)lf.obs.size();
            if (!(lf.obs.size() >= 2 && lf.start < W - 2) || !lf.credible_matching) continue;
            for (size_t k = 0; k < lf.obs.size(); k++) {
                const LineObs &ob = lf.obs[k];
                if (!ob.credible_line || !ob.use_flag || ob.errD > e->cfg.dist_th) continue;
                e->w_lf.push_back(lf.start + (int)k);
                const V3 ps = add(mv(e->Rbw, V3{ob.world[0], ob.world[1], ob.world[2]}), e->Tbw), pe = add(mv(e->Rbw, V3{ob.world[3], ob.world[4], ob.world[5]}), e->Tbw);
                e->w_ld.insert(e->w_ld.end(), ps.begin(), ps.end()); e->w_ld.insert(e->w_ld.end(), pe.begin(), pe.end());
                e->w_ld.insert(e->w_ld.end(), ob.abc, ob.abc + 3);
            }
        }
    }
    double qn[4];
    const double n4 = std::sqrt(e->para_ex[3] * e->para_ex[3] + e->para_ex[4] * e->para_ex[4] + e->para_ex[5] * e->para_ex[5] + e->para_ex[6] * e->para_ex[6]);
    for (int c = 0; c < 4; c++) qn[c] = e->para_ex[3 + c] / n4;
    const M3 Ric = q2R(qn);
    std::memcpy(e->w_Ric, Ric.data(), sizeof e->w_Ric);
    e->w_pk.clear(); e->w_pidx.clear();
    for (auto &b : e->prior_blocks) { e->w_pk.push_back(b.first); e->w_pidx.push_back(b.second); }
    return TCV_OK;
}

void fill_desc(const tcv_estimator *e, tcv_window_desc &d, bool marg, int flag) {
    std::memset(&d, 0, sizeof d);
    tcv_estimator *m = const_cast<tcv_estimator *>(e);
    d.n_frames = W + 1; d.n_landmarks = (int)e->sel.size(); d.estimate_extrinsic = e->cfg.estimate_extrinsic;
    d.para_pose = m->para_pose; d.para_speedbias = m->para_sb; d.para_ex_pose = m->para_ex; d.para_feature = m->para_feature.data();
    d.proj_sqrt_info = e->cfg.focal_length / 1.5; d.proj_loss_a = 1.0; d.line_loss_a = 1.0;
    std::memcpy(d.line_K, e->cfg.K, sizeof d.line_K); std::memcpy(d.line_Ric, e->w_Ric, sizeof d.line_Ric);
    for (int c = 0; c < 3; c++) { d.line_Tic[c] = e->tic[c]; d.gravity[c] = e->cfg.gravity[c]; }
    d.line_exact_jacobian = e->cfg.line_exact_jacobian;
    d.prior = e->prior; d.prior_block_kind = e->w_pk.data(); d.prior_block_index = e->w_pidx.data();
    if (e->estimate_td) { d.para_td = m->para_td; d.proj_td_aux = marg ? e->m_aux.data() : e->w_aux.data(); d.td_TR = e->td_TR; d.td_ROW = e->td_ROW; }      // :1703-1707
    if (!marg) {
        d.n_imu = (int)e->w_imu.size(); d.imu = e->w_imu.data(); d.imu_frame_i = e->w_imu_i.data(); d.imu_frame_j = e->w_imu_j.data();
        d.imu_device = e->w_imu_dev.empty() ? nullptr : e->w_imu_dev.data();      // (entries may be null: that factor's host copy is used)
        d.n_proj = (int)e->w_pi.size(); d.proj_frame_i = e->w_pi.data(); d.proj_frame_j = e->w_pj.data(); d.proj_feature = e->w_pl.data(); d.proj_pts = e->w_pts.data();
        d.n_line = (int)e->w_lf.size(); d.line_frame = e->w_lf.data(); d.line_data = e->w_ld.data();
    } else if (flag == MARGIN_OLD) {
        d.n_imu = (int)e->m_imu.size(); d.imu = e->m_imu.data(); d.imu_frame_i = e->m_imu_i.data(); d.imu_frame_j = e->m_imu_j.data();
        d.imu_device = e->m_imu_dev.empty() ? nullptr : e->m_imu_dev.data();
        d.n_proj = (int)e->m_pi.size(); d.proj_frame_i = e->m_pi.data(); d.proj_frame_j = e->m_pj.data(); d.proj_feature = e->m_pl.data(); d.proj_pts = e->m_pts.data();
    }
}

// factor set and drop sets MarginalizationInfo receives: estimator.cpp:1911-1986 (MARGIN_OLD), :2047-2063 (MARGIN_SECOND_NEW)
void build_marg(tcv_estimator *e, int flag) {
    e->m_imu.clear(); e->m_imu_dev.clear(); e->m_imu_i.clear(); e->m_imu_j.clear(); e->m_pi.clear(); e->m_pj.clear(); e->m_pl.clear(); e->m_pts.clear(); e->m_aux.clear(); e->m_drop.clear();
    if (flag == MARGIN_OLD) {
        for (size_t k = 0; k < e->w_imu.size(); k++)
            if (e->w_imu_i[k] == 0 && e->w_imu[k].sum_dt < 10.0) { e->m_imu.push_back(e->w_imu[k]); e->m_imu_dev.push_back(e->w_imu_dev[k]); e->m_imu_i.push_back(0); e->m_imu_j.push_back(e->w_imu_j[k]); }
        std::vector<int> lms;
        for (size_t k = 0; k < e->w_pi.size(); k++)
            if (e->w_pi[k] == 0) {
                e->m_pi.push_back(0); e->m_pj.push_back(e->w_pj[k]); e->m_pl.push_back(e->w_pl[k]);
                e->m_pts.insert(e->m_pts.end(), e->w_pts.begin() + 6 * k, e->w_pts.begin() + 6 * k + 6);
                if (e->estimate_td) e->m_aux.insert(e->m_aux.end(), e->w_aux.begin() + 8 * k, e->w_aux.begin() + 8 * k + 8);      // :1970-1979: ProjectionTdFactors on para_Td, which is kept
                lms.push_back(e->w_pl[k]);
            }
        std::sort(lms.begin(), lms.end()); lms.erase(std::unique(lms.begin(), lms.end()), lms.end());
        e->m_drop.push_back(e->para_pose); e->m_drop.push_back(e->para_sb);
        for (int l : lms) e->m_drop.push_back(e->para_feature.data() + l);
    } else e->m_drop.push_back(e->para_pose + 7 * (W - 1));
}

// double2vector (:1565-1581; the gauge fix itself ran on the device), setDepth (feature_manager.cpp:379-397)
void apply_states(tcv_estimator *e) {
    for (int i = 0; i <= W; i++) {
        for (int c = 0; c < 3; c++) { e->Ps[i][c] = e->para_pose[7 * i + c]; e->Vs[i][c] = e->para_sb[9 * i + c]; e->Bas[i][c] = e->para_sb[9 * i + 3 + c]; e->Bgs[i][c] = e->para_sb[9 * i + 6 + c]; }
        e->Rs[i] = q2R(e->para_pose + 7 * i + 3);
    }
    for (int c = 0; c < 3; c++) e->tic[c] = e->para_ex[c];
    e->ric = q2R(e->para_ex + 3);
    if (e->estimate_td) e->td = e->para_td[0];      // :1601-1602
    for (size_t l = 0; l < e->sel.size(); l++) {
        Feature &f = e->features[e->sel[l]];
        f.depth = 1.0 / e->para_feature[l];
        f.solve_flag = f.depth < 0 ? 2 : 1;
    }
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
    T.imu = e->w_imu; T.imu_i = e->w_imu_i; T.imu_j = e->w_imu_j;
    for (size_t k = 0; k < T.imu.size(); k++)
        if (k < e->w_imu_dev.size() && e->w_imu_dev[k]) { const int rc = tcv_preint_export(e->w_imu_dev[k], &T.imu[k]); if (rc != TCV_OK) return rc; }
    T.pi = e->w_pi; T.pj = e->w_pj; T.pl = e->w_pl; T.pts = e->w_pts; T.lf = e->w_lf; T.ld = e->w_ld;
    T.aux = e->w_aux; T.td_in = e->estimate_td ? e->para_td[0] : 0.0; T.td_out = 0.0;
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

bool failure_detection(const tcv_estimator *e) {
    if (nrm(e->Bas[W]) > 2.5 || nrm(e->Bgs[W]) > 1.0) return true;
    if (e->have_last) {
        if (nrm(sub(e->Ps[W], e->last_P)) > 5 || std::fabs(e->Ps[W][2] - e->last_P[2]) > 1) return true;
    }
    return false;
}

void new_buf(tcv_estimator *e, int j) {
    ImuBuf &b = e->bufs[j];
    b.valid = true; b.acc0 = e->acc_0; b.gyr0 = e->gyr_0; b.ba = e->Bas[j]; b.bg = e->Bgs[j]; b.acc.clear(); b.gyr.clear();
}

void slide_window(tcv_estimator *e) {
    if (e->frame_count != W) return;
    if (e->marg_flag == MARGIN_OLD) {
        const M3 back_R0 = e->Rs[0];
        const V3 back_P0 = e->Ps[0];
        for (int i = 0; i < W; i++) {      // the swaps of :2131-2153 followed by the copy of slot W-1 into W
            e->Ps[i] = e->Ps[i + 1]; e->Rs[i] = e->Rs[i + 1]; e->Vs[i] = e->Vs[i + 1]; e->Bas[i] = e->Bas[i + 1]; e->Bgs[i] = e->Bgs[i + 1];
            // (moves, not copies: this runs once per frame and estimator on the host's critical path; slot W is refilled right below --
            // except the line bookkeeping, whose slot W keeps its content: WorldLinesInFOV[W] = WorldLinesInFOV[W-1], :2158)
            e->serials[i] = e->serials[i + 1];
            e->bufs[i] = std::move(e->bufs[i + 1]); e->pre[i] = e->pre[i + 1]; e->preh[i] = std::move(e->preh[i + 1]); e->pre_valid[i] = e->pre_valid[i + 1];
            if (i + 1 < W) { e->line_obs[i] = std::move(e->line_obs[i + 1]); e->fov[i] = std::move(e->fov[i + 1]); }
            else { e->line_obs[i] = e->line_obs[i + 1]; e->fov[i] = e->fov[i + 1]; }
        }
        e->pre_valid[W] = false;
        e->serials[W] = -1;
        new_buf(e, W);
        // slideWindowOld (:2242-2259) -> removeBackShiftDepth (feature_manager.cpp:559-616)
        const M3 R0 = mm(back_R0, e->ric), R1 = mm(e->Rs[0], e->ric);
        const V3 P0 = add(back_P0, mv(back_R0, e->tic)), P1 = add(e->Ps[0], mv(e->Rs[0], e->tic));
        std::vector<Feature> kept;
        for (auto &f : e->features) {
            if (f.start != 0) { f.start -= 1; kept.push_back(std::move(f)); continue; }
            const V3 uv_i = f.obs.front();
            f.obs.erase(f.obs.begin());
            if (!f.aux.empty()) f.aux.erase(f.aux.begin());
            if (f.obs.size() < 2) continue;
            const V3 pts_j = mv(tr(R1), sub(add(mv(R0, scl(uv_i, f.depth)), P0), P1));
            f.depth = pts_j[2] > 0 ? pts_j[2] : e->cfg.init_depth;
            kept.push_back(std::move(f));
        }
        e->features.swap(kept);
        std::vector<LineFeature> keptl;                // line features: feature_manager.cpp:598-614
        for (auto &lf : e->linefeatures) {
            if (lf.start != 0) { lf.start -= 1; keptl.push_back(std::move(lf)); continue; }
            lf.obs.erase(lf.obs.begin());
            if (!lf.obs.empty()) keptl.push_back(std::move(lf));
        }
        e->linefeatures.swap(keptl);
    } else {
        // MARGIN_SECOND_NEW (:2189-2230): the newest frame replaces the second newest, their IMU buffers are concatenated
        ImuBuf &a = e->bufs[W - 1], &b = e->bufs[W];
        a.acc.insert(a.acc.end(), b.acc.begin(), b.acc.end()); a.gyr.insert(a.gyr.end(), b.gyr.begin(), b.gyr.end());
        e->pre_valid[W - 1] = false;
        e->Ps[W - 1] = e->Ps[W]; e->Rs[W - 1] = e->Rs[W]; e->Vs[W - 1] = e->Vs[W]; e->Bas[W - 1] = e->Bas[W]; e->Bgs[W - 1] = e->Bgs[W];
        e->line_obs[W - 1] = e->line_obs[W];
        e->serials[W - 1] = e->serials[W]; e->serials[W] = -1;
        new_buf(e, W);
        e->pre_valid[W] = false;
        std::vector<Feature> kept;                     // slideWindowNew -> removeFront(frame_count) (feature_manager.cpp:655-675)
        for (auto &f : e->features) {
            if (f.start == W) { f.start -= 1; kept.push_back(std::move(f)); continue; }
            if (f.end() < W - 1) { kept.push_back(std::move(f)); continue; }
            f.obs.erase(f.obs.begin() + (W - 1 - f.start));
            if (!f.aux.empty()) f.aux.erase(f.aux.begin() + (W - 1 - f.start));
            if (!f.obs.empty()) kept.push_back(std::move(f));
        }
        e->features.swap(kept);
        std::vector<LineFeature> keptl;                // feature_manager.cpp:677-695
        for (auto &lf : e->linefeatures) {
            if (lf.start == W) { lf.start -= 1; keptl.push_back(std::move(lf)); continue; }
            if (lf.start + (int)lf.obs.size() - 1 < W - 1) { keptl.push_back(std::move(lf)); continue; }
            lf.obs.erase(lf.obs.begin() + (W - 1 - lf.start));
            if (!lf.obs.empty()) keptl.push_back(std::move(lf));
        }
        e->linefeatures.swap(keptl);
        e->fov[W - 1] = e->fov[W];
    }
    std::vector<Feature> ok;                           // removeFailures (:399-408)
    for (auto &f : e->features) if (f.solve_flag != 2) ok.push_back(std::move(f));
    e->features.swap(ok);
}

}  // namespace

static void clear_state(tcv_estimator *e) {
    const tcv_estimator_config *cfg = &e->cfg;
    for (int i = 0; i <= W; i++) {
        e->Ps[i] = e->Vs[i] = e->Bas[i] = e->Bgs[i] = V3{0, 0, 0}; e->Rs[i] = eye(); e->pre_valid[i] = false; std::memset(&e->pre[i], 0, sizeof e->pre[i]); e->preh[i].reset();
        e->bufs[i] = ImuBuf(); e->line_obs[i].clear(); e->fov[i].clear();
    }
    for (int c = 0; c < 3; c++) e->tic[c] = cfg->tic[c];
    std::memcpy(e->ric.data(), cfg->ric, sizeof(double) * 9);
    std::memset(&e->stats, 0, sizeof e->stats);
    e->features.clear(); e->linefeatures.clear(); e->fov_ready = false;
    if (e->prior) { tcv_prior_destroy(e->prior); e->prior = nullptr; }
    e->prev.reset(); e->prev_k = -1;
    e->pend.reset(); e->pend_k = -1;
    e->prior_blocks.clear();
    e->frame_count = 0; e->marg_flag = MARGIN_OLD;
    e->have_acc0 = false; e->have_last = false;
    e->acc_0 = e->gyr_0 = e->last_P = V3{0, 0, 0};
    e->para_feature.clear(); e->sel.clear();
    e->td = e->td0; e->para_td[0] = e->td0; e->staged_aux.clear(); e->staged_n = -1;      // td = TD (estimator.cpp:51, :170)
    e->n_line_obs_total = 0; e->phase = 0; e->opt_failed = 0; e->opt_msg.clear(); e->pend_failed = 0; e->pend_msg.clear();
    // relocalization_info = 0, drift_correct_r = Identity, drift_correct_t = Zero (estimator.cpp:185-188); the serials restart
    e->next_serial = 0;
    for (int i = 0; i <= W; i++) e->serials[i] = -1;
    e->relo_pending = false; e->relo_match.clear(); e->w_relo = false; e->r_pi.clear(); e->r_pl.clear(); e->r_pts.clear();
    std::memset(&e->relo_out, 0, sizeof e->relo_out);
    e->relo_out.drift_correct_r[0] = e->relo_out.drift_correct_r[4] = e->relo_out.drift_correct_r[8] = 1.0;
}
extern "C" int tcv_estimator_create(tcv_estimator **out, const tcv_estimator_config *cfg) {
    if (!out || !cfg || !(cfg->imu_dt > 0) || !(cfg->focal_length > 0) || cfg->num_iterations < 1) { tcv::set_error("estimator_create: bad configuration"); return TCV_ERR_INVALID; }
    tcv_estimator *e = new tcv_estimator();
    e->cfg = *cfg;
    clear_state(e);
    *out = e;
    return TCV_OK;
}
// Estimator::clearState() + setParameter() (estimator.cpp:126-189, :39-52): what estimator_node.cpp does after failureDetection fired
// (:437-446) or on a restart request -- window, IMU buffers, pre-integrations, feature and line tracks, the marginalisation prior and the
// biases are dropped, the extrinsic goes back to the configured one; the line map (setParameters, :54-124) stays.
extern "C" int tcv_estimator_reset(tcv_estimator *e) {
    if (!e) return TCV_ERR_INVALID;
    clear_state(e);
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
// the same for tasks that can fail: every task's code and, where it failed, the error text of the thread it ran on (the text is per thread)
struct TaskRc { int rc = TCV_OK; std::string msg; };
std::vector<TaskRc> for_each_estimator_rc(int n, const std::function<int(int)> &fn, bool on_caller = false) {
    std::vector<TaskRc> r(n);
    auto one = [&](int i) { r[i].rc = fn(i); if (r[i].rc != TCV_OK) r[i].msg = tcv_last_error(); };
    if (on_caller) for (int i = 0; i < n; i++) one(i); else for_each_estimator(n, one);
    return r;
}
// the first failure in index order, its text on the calling thread; rcs_out (one int per task), when given, takes every code
int first_failure(const std::vector<TaskRc> &r, int *rcs_out = nullptr) {
    if (rcs_out) for (size_t i = 0; i < r.size(); i++) rcs_out[i] = r[i].rc;
    for (const TaskRc &t : r) if (t.rc != TCV_OK) { tcv::set_error(t.msg); return t.rc; }
    return TCV_OK;
}
}  // namespace
extern "C" int tcv_estimators_begin_frames(tcv_estimator *const *es, int n, const tcv_frame_input *in, int *ready, int *rc_out) {
    if (!es || n <= 0 || !in || !ready) { tcv::set_error("estimators_begin_frames: bad argument"); return TCV_ERR_INVALID; }
    for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (es[i] == es[j]) { tcv::set_error("estimators_begin_frames: the same estimator twice"); return TCV_ERR_INVALID; }
    return first_failure(for_each_estimator_rc(n, [&](int i) {
        const tcv_frame_input &f = in[i];
        ready[i] = 0;
        return tcv_estimator_begin_frame(es[i], f.n_imu, f.acc, f.gyr, f.n_points, f.point_ids, f.points, f.n_lines, f.line_ids, f.lines, f.truth, &ready[i]);
    }), rc_out);
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
    fill_desc(e, d, true, e->marg_flag);
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
        fill_desc(e, d, false, e->marg_flag);
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
        const double per = 8.0 * ((77 + 99 + 7 + L) + 287.0 * e->w_imu.size() + 6.0 * e->w_pi.size() + 9.0 * e->w_lf.size() + 21 + (pn > 0 ? pn * pn + pn + 86 : 0))
                           + 4.0 * (4.0 * e->w_imu.size() + 4.0 * e->w_pi.size() + e->w_lf.size()) + 8.0 * ((171 + L) + 1);
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
        e->stats.marg_flag = e->marg_flag; e->stats.n_landmarks = (int)e->sel.size(); e->stats.n_proj = (int)e->w_pi.size(); e->stats.n_line = (int)e->w_lf.size();
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
extern "C" int tcv_estimator_get_window_snapshot(const tcv_estimator *e, tcv_window_snapshot *o) {
    if (!e || !o) return TCV_ERR_INVALID;
    const WindowTap &T = e->tap;
    if (!T.on || !T.have) { tcv::set_error("estimator_get_window_snapshot: no snapshot (tap off, or no window optimised since it was switched on)"); return TCV_ERR_INVALID; }
    std::memset(o, 0, sizeof *o);
    o->n_frames = W + 1; o->n_landmarks = (int)T.feat_in.size(); o->n_imu = (int)T.imu.size(); o->n_proj = (int)T.pi.size(); o->n_line = (int)T.lf.size();
    o->marg_flag = T.marg_flag; o->estimate_extrinsic = e->cfg.estimate_extrinsic; o->line_exact_jacobian = e->cfg.line_exact_jacobian;
    o->pose_in = T.pose_in.data(); o->speedbias_in = T.sb_in.data(); o->ex_pose_in = T.ex_in.data(); o->feature_in = T.feat_in.data();
    o->pose_out = T.pose_out.data(); o->speedbias_out = T.sb_out.data(); o->ex_pose_out = T.ex_out.data(); o->feature_out = T.feat_out.data();
    o->imu = T.imu.data(); o->imu_frame_i = T.imu_i.data(); o->imu_frame_j = T.imu_j.data();
    o->proj_frame_i = T.pi.data(); o->proj_frame_j = T.pj.data(); o->proj_feature = T.pl.data(); o->proj_pts = T.pts.data();
    o->line_frame = T.lf.data(); o->line_data = T.ld.data();
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
    if (!e || !o) return TCV_ERR_INVALID;
    const WindowTap &T = e->tap;
    if (!T.on || !T.have) { tcv::set_error("estimator_get_window_snapshot_td: no snapshot (tap off, or no window optimised since it was switched on)"); return TCV_ERR_INVALID; }
    std::memset(o, 0, sizeof *o);
    o->estimate_td = e->estimate_td; o->n_proj = (int)T.pi.size();
    o->td_in = T.td_in; o->td_out = T.td_out; o->TR = e->td_TR; o->ROW = e->td_ROW;
    o->proj_td_aux = T.aux.empty() ? nullptr : T.aux.data();
    return TCV_OK;
}
extern "C" int tcv_estimator_get_window_snapshot_relo(const tcv_estimator *e, tcv_window_snapshot_relo *o) {
    if (!e || !o) return TCV_ERR_INVALID;
    const WindowTap &T = e->tap;
    if (!T.on || !T.have) { tcv::set_error("estimator_get_window_snapshot_relo: no snapshot (tap off, or no window optimised since it was switched on)"); return TCV_ERR_INVALID; }
    std::memset(o, 0, sizeof *o);
    if (!T.has_relo) return TCV_OK;
    o->has_relo = 1; o->local_index = T.relo_local; o->n_relo = (int)T.r_pi.size(); o->frame_index = T.relo_frame_index; o->frame_serial = T.relo_frame_serial;
    std::memcpy(o->relo_pose_in, T.relo_in, sizeof o->relo_pose_in); std::memcpy(o->relo_pose_out, T.relo_out, sizeof o->relo_pose_out);
    o->relo_frame_i = T.r_pi.data(); o->relo_feature = T.r_pl.data(); o->relo_pts = T.r_pts.data();
    std::memcpy(o->prev_relo_t, T.relo_prev, sizeof o->prev_relo_t); std::memcpy(o->prev_relo_r, T.relo_prev + 3, sizeof o->prev_relo_r);
    o->result = T.relo_result;
    return TCV_OK;
}
extern "C" int tcv_estimator_get_stats(const tcv_estimator *e, tcv_estimator_stats *out) {
    if (!e || !out) return TCV_ERR_INVALID;
    *out = e->stats;
    return TCV_OK;
}
