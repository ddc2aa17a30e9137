// Native estimator: the device-free bookkeeping of a window -- IMU propagation, feature and line tracks, triangulation, the window's
// parameter blocks and factor lists, the marginalisation problem's, and the slide.
// Reference: vins_estimator/src/estimator.cpp (processIMU :191-228, vector2double :1492-1535, double2vector :1537-1627, failureDetection
// :1629-1675, slideWindowWithLinesFoV :2121-2259) and feature_manager.cpp (addFeaturesCheckParallax :260-334, setDepth :379-397,
// removeFailures :399-408, triangulate :440-492, removeLineOutlier :494-534, removeBackShiftDepth :559-616, removeFront :655-696,
// compensatedParallax2 :698-734).
// Plain host C++: no HIP header, no call into the library -- tests/dev/est_tracks_sanitize.cpp compiles this file alone under ASan + UBSan.
#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "tcv_est.h"

namespace tcv_est {

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

static bool selected(const Feature &f) { return f.obs.size() >= 2 && f.start < W - 2; }

// smallest right singular vector of A (rows x 4): one-sided Jacobi on the columns (what JacobiSVD in triangulate() delivers)
static void smallest_right_singular_vector(std::vector<std::array<double, 4>> A, double v_out[4]) {
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

// removeLineOutlier (feature_manager.cpp:494-534), as processImagewithLine runs it behind updateLinePairInWindow (estimator.cpp:328-336)
void remove_line_outlier(tcv_estimator *e) {
    for (auto &lf : e->linefeatures) {
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
    FactorLists &w = e->w;
    w.clear();
    for (int k = 0; k < W; k++)
        if (e->pre[k + 1].sum_dt <= 10.0) {      // estimator.cpp:1726
            w.imu.push_back(e->pre[k + 1]); w.imu_i.push_back(k); w.imu_j.push_back(k + 1);
            w.imu_dev.push_back(e->preh[k + 1].get());
        }
    for (size_t l = 0; l < e->sel.size(); l++) {      // estimator.cpp:1737-1771
        const Feature &f = e->features[e->sel[l]];
        for (size_t k = 1; k < f.obs.size(); k++) {
            w.pi.push_back(f.start); w.pj.push_back(f.start + (int)k); w.pl.push_back((int)l);
            w.pts.insert(w.pts.end(), f.obs[0].begin(), f.obs[0].end()); w.pts.insert(w.pts.end(), f.obs[k].begin(), f.obs[k].end());
            if (e->estimate_td) {      // the constructor arguments of ProjectionTdFactor (:1757-1763): velocities, cur_td, uv.y() of the anchor and of observation k
                const std::array<double, 5> &a = f.aux[0], &b = f.aux[k];
                const double x[8] = {a[2], a[3], b[2], b[3], a[4], b[4], a[1], b[1]};
                w.aux.insert(w.aux.end(), x, x + 8);
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
    e->n_line_obs_total = 0;
    if (!e->assoc) {
        for (int i = 0; i <= W; i++) for (auto &g : e->line_obs[i]) { w.lf.push_back(i); w.ld.insert(w.ld.end(), g.d, g.d + 9); }
    } else {      // estimator.cpp:1786-1846
        for (auto &lf : e->linefeatures) {
            e->n_line_obs_total += (int)lf.obs.size();
            if (!(lf.obs.size() >= 2 && lf.start < W - 2) || !lf.credible_matching) continue;
            for (size_t k = 0; k < lf.obs.size(); k++) {
                const LineObs &ob = lf.obs[k];
                if (!ob.credible_line || !ob.use_flag || ob.errD > e->cfg.dist_th) continue;
                w.lf.push_back(lf.start + (int)k);
                const V3 ps = add(mv(e->Rbw, V3{ob.world[0], ob.world[1], ob.world[2]}), e->Tbw), pe = add(mv(e->Rbw, V3{ob.world[3], ob.world[4], ob.world[5]}), e->Tbw);
                w.ld.insert(w.ld.end(), ps.begin(), ps.end()); w.ld.insert(w.ld.end(), pe.begin(), pe.end());
                w.ld.insert(w.ld.end(), ob.abc, ob.abc + 3);
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

// factor set and drop sets MarginalizationInfo receives: estimator.cpp:1911-1986 (MARGIN_OLD: the window's IMU and projection factors on
// frame 0, never its line factors), :2047-2063 (MARGIN_SECOND_NEW: no factors, only the prior)
void build_marg(tcv_estimator *e, int flag) {
    const FactorLists &w = e->w;
    FactorLists &m = e->m;
    m.clear(); e->m_drop.clear();
    if (flag != MARGIN_OLD) { e->m_drop.push_back(e->para_pose + 7 * (W - 1)); return; }
    for (size_t k = 0; k < w.imu.size(); k++)
        if (w.imu_i[k] == 0 && w.imu[k].sum_dt < 10.0) { m.imu.push_back(w.imu[k]); m.imu_dev.push_back(w.imu_dev[k]); m.imu_i.push_back(0); m.imu_j.push_back(w.imu_j[k]); }
    std::vector<int> lms;
    for (size_t k = 0; k < w.pi.size(); k++)
        if (w.pi[k] == 0) {
            m.pi.push_back(0); m.pj.push_back(w.pj[k]); m.pl.push_back(w.pl[k]);
            m.pts.insert(m.pts.end(), w.pts.begin() + 6 * k, w.pts.begin() + 6 * k + 6);
            if (e->estimate_td) m.aux.insert(m.aux.end(), w.aux.begin() + 8 * k, w.aux.begin() + 8 * k + 8);      // :1970-1979: ProjectionTdFactors on para_Td, which is kept
            lms.push_back(w.pl[k]);
        }
    std::sort(lms.begin(), lms.end()); lms.erase(std::unique(lms.begin(), lms.end()), lms.end());
    e->m_drop.push_back(e->para_pose); e->m_drop.push_back(e->para_sb);
    for (int l : lms) e->m_drop.push_back(e->para_feature.data() + l);
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

bool failure_detection(const tcv_estimator *e) {
    if (nrm(e->Bas[W]) > 2.5 || nrm(e->Bgs[W]) > 1.0) return true;
    if (e->have_last) {
        if (nrm(sub(e->Ps[W], e->last_P)) > 5 || std::fabs(e->Ps[W][2] - e->last_P[2]) > 1) return true;
    }
    return false;
}

static void new_buf(tcv_estimator *e, int j) {
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

}  // namespace tcv_est
