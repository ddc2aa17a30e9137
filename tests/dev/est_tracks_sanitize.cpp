// Developer tool, host only: the native estimator's device-free bookkeeping (tc-viml_amd/csrc/tcv_est_tracks.cpp) under AddressSanitizer
// and UndefinedBehaviorSanitizer, as a stand-alone executable that needs neither a device nor the library.  Two estimator states -- one with
// given line observations, one with line tracks whose association results are filled in by hand -- are driven through 55 frames (45 full
// windows) the way tcv_estimator_begin_frame / tcv_estimators_optimize / tcv_estimator_finish_frame drive them, with a stand-in for the
// device (pre-integration: sum_dt only; solve: the parameter blocks stay, one inverse depth is made negative every seventh window).  Point
// tracks of 1 to 14 frames are born and end all the time and cross slot W - 1, every observation carries its ESTIMATE_TD aux, and the
// keyframe decision is forced to OLD OLD NEW OLD NEW NEW ..., which holds the four orders of two slides.  Between frames build_window and
// build_marg (both flags) run; after every frame the program checks the tracks' and the factor lists' own invariants.  Exits 0.  From the
// repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       tests/dev/est_tracks_sanitize.cpp tc-viml_amd/csrc/tcv_est_tracks.cpp -o /tmp/est_tracks_sanitize && /tmp/est_tracks_sanitize
#include <cstdio>
#include <memory>
#include <vector>

#include "../../tc-viml_amd/csrc/tcv_est.h"

using namespace tcv_est;

#define CHECK(x)                                                                                        \
    do {                                                                                                \
        if (!(x)) { std::printf("FAILED %s (line %d, frame %d)\n", #x, __LINE__, g_frame); return 1; } \
    } while (0)

static int g_frame = 0;
static const double DT = 0.005, SPEED = 1.0;
static const int N_IMU = 20, N_FRAMES = 55;

static bool lists_agree(const FactorLists &f, bool td, bool lines_allowed, int n_landmarks) {
    const size_t ni = f.imu.size(), np = f.pi.size(), nl = f.lf.size();
    if (f.imu_dev.size() != ni || f.imu_i.size() != ni || f.imu_j.size() != ni) return false;
    if (f.pj.size() != np || f.pl.size() != np || f.pts.size() != 6 * np || f.aux.size() != (td ? 8 * np : 0)) return false;
    if (f.ld.size() != 9 * nl || (!lines_allowed && nl != 0)) return false;
    for (size_t k = 0; k < ni; k++) if (f.imu_i[k] < 0 || f.imu_j[k] != f.imu_i[k] + 1 || f.imu_j[k] > W) return false;
    for (size_t k = 0; k < np; k++) if (f.pi[k] < 0 || f.pj[k] <= f.pi[k] || f.pj[k] > W || f.pl[k] < 0 || f.pl[k] >= n_landmarks) return false;
    for (size_t k = 0; k < nl; k++) if (f.lf[k] < 0 || f.lf[k] > W) return false;
    return true;
}

static int tracks_ok(const tcv_estimator *e) {
    for (const Feature &f : e->features) { CHECK(f.start >= 0 && !f.obs.empty() && f.start + (int)f.obs.size() <= W + 1); CHECK(f.aux.size() == f.obs.size()); }
    for (const LineFeature &lf : e->linefeatures) CHECK(lf.start >= 0 && !lf.obs.empty() && lf.start + (int)lf.obs.size() <= W + 1);
    return 0;
}

static int drops_ok(const tcv_estimator *e, int flag) {
    CHECK(!e->m_drop.empty());
    if (flag == MARGIN_SECOND_NEW) { CHECK(e->m_drop.size() == 1 && e->m_drop[0] == e->para_pose + 7 * (W - 1)); CHECK(e->m.imu.empty() && e->m.pi.empty() && e->m.lf.empty()); }
    for (const double *p : e->m_drop) {
        const bool in_pose = p >= e->para_pose && p < e->para_pose + (W + 1) * 7, in_sb = p >= e->para_sb && p < e->para_sb + (W + 1) * 9;
        const bool in_feat = p >= e->para_feature.data() && p < e->para_feature.data() + e->para_feature.size();
        CHECK(in_pose || in_sb || in_feat);
    }
    for (size_t k = 0; k < e->m.pi.size(); k++) CHECK(e->m.pi[k] == 0);
    for (size_t k = 0; k < e->m.imu_i.size(); k++) CHECK(e->m.imu_i[k] == 0);
    return 0;
}

static int drive(bool assoc) {
    std::unique_ptr<tcv_estimator> owner(new tcv_estimator());
    tcv_estimator *e = owner.get();
    tcv_estimator_config &c = e->cfg;
    c.focal_length = 460.0; c.min_parallax = 10.0 / 460.0; c.init_depth = 5.0; c.gravity[2] = 9.81; c.imu_dt = DT; c.dist_th = 50.0;
    c.ric[0] = c.ric[4] = c.ric[8] = 1.0; c.estimate_extrinsic = 1; c.num_iterations = 8;
    e->ric = eye();
    e->assoc = assoc; e->Rbw = eye();
    e->estimate_td = 1; e->td0 = e->td = 0.01; e->td_ROW = 480.0;

    int pairs[2][2] = {{0, 0}, {0, 0}}, prev_flag = -1, n_windows = 0, n_failures = 0, n_shrunk = 0, n_across = 0, n_line_outliers = 0, n_line_factors = 0;
    static const int pattern[6] = {MARGIN_OLD, MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_SECOND_NEW};
    for (int k = 0; k < N_FRAMES; k++) {
        g_frame = k;
        // ---- the frame's inputs: IMU of a camera that moves along x at SPEED, the point tracks alive at frame k, its lines
        std::vector<double> acc(3 * (N_IMU + 1), 0.0), gyr(3 * (N_IMU + 1), 0.0);
        for (int i = 0; i <= N_IMU; i++) acc[3 * i + 2] = 9.81;
        const double px = SPEED * DT * N_IMU * k;
        std::vector<int> ids, line_ids;
        std::vector<double> pts, aux4, lines;
        for (int f = 0; f <= 3 * k + 2; f++) {      // three tracks are born per frame; track f lives 1 + f % 14 frames
            const int birth = f / 3, len = 1 + f % 14;
            if (k < birth || k >= birth + len) continue;
            const double X[3] = {SPEED * DT * N_IMU * birth + (f % 5 - 2) * 0.3, (f % 3 - 1) * 0.2, 3.0 + f % 4};
            ids.push_back(f);
            const double u = (X[0] - px) / X[2], v = X[1] / X[2];
            pts.insert(pts.end(), {u, v, 1.0});
            aux4.insert(aux4.end(), {460.0 * u + 376.0, 460.0 * v + 240.0, -SPEED / X[2], 0.0});
        }
        for (int l = 0; l <= 2 * k + 1; l++) {      // two line tracks are born per frame; track l lives 1 + l % 12 frames
            const int birth = l / 2, len = 1 + l % 12;
            if (k < birth || k >= birth + len) continue;
            if (assoc) { line_ids.push_back(l); lines.insert(lines.end(), {10.0 + l % 50, 20.0, 60.0 + l % 50, 25.0 + k % 3}); }
            else if (l % 4 == 0) lines.insert(lines.end(), {px + 1.0, -1.0, 4.0, px + 1.0, 1.0, 4.0, 0.0, 1.0, -0.1 * (l % 3)});
        }
        // ---- tcv_estimator_begin_frame
        const int fc = e->frame_count;
        e->serials[fc] = e->next_serial++;
        process_imu(e, N_IMU, acc.data(), gyr.data());
        const bool old = add_features_check_parallax(e, (int)ids.size(), ids.data(), pts.data(), aux4.data(), (int)(assoc ? line_ids.size() : lines.size() / 9), line_ids.data(), lines.data());
        (void)old;
        if (k <= W) { e->Ps[fc] = V3{px, 0, 0}; e->Vs[fc] = V3{SPEED, 0, 0}; e->Rs[fc] = eye(); }
        CHECK(tracks_ok(e) == 0);
        if (fc < W) {
            e->frame_count++;
            const int j = e->frame_count;
            e->Bas[j] = e->Bas[j - 1]; e->Bgs[j] = e->Bgs[j - 1]; e->Ps[j] = e->Ps[j - 1]; e->Rs[j] = e->Rs[j - 1]; e->Vs[j] = e->Vs[j - 1];
            continue;
        }
        e->marg_flag = pattern[n_windows % 6];
        if (prev_flag >= 0) pairs[prev_flag][e->marg_flag]++;
        prev_flag = e->marg_flag;
        // ---- tcv_estimators_optimize, the device's part stood in for
        for (int j = 1; j <= W; j++) if (!e->pre_valid[j]) { CHECK(e->bufs[j].valid && e->bufs[j].acc.size() == e->bufs[j].gyr.size()); e->pre[j].sum_dt = DT * (double)e->bufs[j].acc.size(); e->pre_valid[j] = true; }
        if (assoc) {
            for (LineFeature &lf : e->linefeatures)
                for (size_t o = 0; o < lf.obs.size(); o++) {      // what assoc_finish writes: every fifth track with a second direction on its odd observations
                    LineObs &ob = lf.obs[o];
                    const bool other = lf.id % 5 == 0 && o % 2 == 1;
                    const double wl[6] = {1.0 + lf.id, 0.0, 4.0, 1.0 + lf.id + (other ? 0.0 : 1.0), other ? 1.0 : 0.0, 4.0};
                    for (int i = 0; i < 6; i++) ob.world[i] = wl[i];
                    ob.errA = 0.01; ob.errD = lf.id % 7 == 0 ? 100.0 : 1.0; ob.overlap = 0.9; ob.use_flag = true; ob.credible_line = true;
                }
            remove_line_outlier(e);
            for (const LineFeature &lf : e->linefeatures) for (const LineObs &ob : lf.obs) n_line_outliers += ob.credible_line ? 0 : 1;      // (credible_matching itself never falls: count / size is an integer division, as in the reference)
        }
        triangulate(e);
        CHECK(build_window(e) == TCV_OK);
        const int nl = (int)e->sel.size();
        CHECK(lists_agree(e->w, true, true, nl) && (int)e->para_feature.size() == (nl > 1 ? nl : 1));
        CHECK(e->w_pk.size() == e->w_pidx.size());
        n_line_factors += (int)e->w.lf.size();
        for (const Feature &f : e->features) n_across += f.start < W - 1 && f.end() >= W - 1 ? 1 : 0;
        for (int flag = 1; flag >= -1; flag--) {      // both flags, then the frame's own (what the slide below follows)
            const int fl = flag < 0 ? e->marg_flag : flag;
            build_marg(e, fl);
            CHECK(lists_agree(e->m, true, false, nl) && drops_ok(e, fl) == 0);
        }
        if (n_windows % 7 == 3 && nl > 0) { e->para_feature[0] = -0.5; n_failures++; }      // a negative depth: solve_flag 2, removeFailures
        apply_states(e);
        // ---- tcv_estimator_finish_frame
        CHECK(!failure_detection(e));
        if (e->marg_flag == MARGIN_OLD) for (const Feature &f : e->features) n_shrunk += f.start == 0 && f.obs.size() == 2 ? 1 : 0;
        const size_t before = e->features.size();
        slide_window(e);
        e->last_P = e->Ps[W]; e->have_last = true;
        CHECK(e->features.size() <= before && tracks_ok(e) == 0);
        for (const Feature &f : e->features) CHECK(f.solve_flag != 2);
        for (int i = 0; i < W; i++) CHECK(e->serials[i] >= 0);
        CHECK(e->serials[W] == -1 && e->bufs[W].valid && e->bufs[W].acc.empty() && !e->pre_valid[W]);
        n_windows++;
    }
    CHECK(n_windows >= 40 && pairs[0][0] > 0 && pairs[0][1] > 0 && pairs[1][0] > 0 && pairs[1][1] > 0);
    CHECK(n_failures > 0 && n_shrunk > 0 && n_across > 0);
    if (assoc) CHECK(n_line_outliers > 0 && n_line_factors > 0 && !e->linefeatures.empty());
    else CHECK(n_line_factors > 0);
    std::printf("%s lines: %d windows, slides OLD>OLD %d OLD>NEW %d NEW>OLD %d NEW>NEW %d, %d negative depths, %d tracks shrunk away, %d line factors, %d outlier line observations\n",
                assoc ? "associated" : "given", n_windows, pairs[0][0], pairs[0][1], pairs[1][0], pairs[1][1], n_failures, n_shrunk, n_line_factors, n_line_outliers);
    return 0;
}

int main() {
    if (drive(false) || drive(true)) return 1;
    std::printf("ok\n");
    return 0;
}
