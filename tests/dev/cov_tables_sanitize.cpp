// Developer tool, host only: the covariance table builders (tc-viml_amd/csrc/tcv_cov_tables.cpp) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone executable.  One synthetic window -- 4 frames, 3 IMU factors, 7 landmarks with one to three
// point factors each, 2 line factors -- goes through pack_problem (no device is touched), then through the owner lists, the landmark slot
// walk, the slot table and the request tables; the program checks the tables' own invariants and exits 0.  From the repository root:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       tests/dev/cov_tables_sanitize.cpp tc-viml_amd/csrc/tcv_cov_tables.cpp -fsanitize=address,undefined \
//       -Ltc-viml_amd -ltcv_hip -Wl,-rpath,$PWD/tc-viml_amd -o /tmp/cov_tables_sanitize && /tmp/cov_tables_sanitize
//
// Only this file and the builders are instrumented; the problem, the packer and the error text come from the library as built.
#include <cstdio>
#include <vector>

#include "../../include/tcv_covariance.h"
#include "../../tc-viml_amd/csrc/tcv_cov.h"
#include "../../tc-viml_amd/csrc/tcv_host.h"

using namespace tcv;

#define CHECK(x)                                                                                          \
    do {                                                                                                  \
        if (!(x)) { std::printf("FAILED %s (line %d): %s\n", #x, __LINE__, tcv_last_error()); return 1; } \
    } while (0)

int main() {
    enum { F = 4, L = 7 };
    double pose[F][7], sb[F][9] = {}, ex[7] = {0.01, 0.02, 0.03, 0, 0, 0, 1}, lam[L];
    for (int i = 0; i < F; i++) { const double q[7] = {0.3 * i, 0.02 * i, 0.01 * i, 0, 0, 0, 1}; std::copy(q, q + 7, pose[i]); sb[i][0] = 0.3; }
    for (int l = 0; l < L; l++) lam[l] = 0.2 + 0.01 * l;
    std::vector<tcv_imu_preintegration> imu(F - 1);
    std::vector<int> fi, fj;
    for (int i = 0; i + 1 < F; i++) {
        tcv_imu_preintegration q = {};
        q.delta_p[0] = 0.3; q.delta_q[3] = 1.0; q.delta_v[0] = 0.0; q.sum_dt = 1.0;
        for (int d = 0; d < 15; d++) { q.jacobian[16 * d] = 1.0; q.covariance[16 * d] = 1e-4; }
        imu[i] = q; fi.push_back(i); fj.push_back(i + 1);
    }
    std::vector<int> pf_i, pf_j, pf_l;
    std::vector<double> pts;
    for (int l = L - 1; l >= 0; l--)      // landmarks in another order than their registration, frames i < j of every kind
        for (int k = 0; k <= l % 3; k++) {
            const int a = l % 2, b = a + 1 + k > F - 1 ? F - 1 : a + 1 + k;
            pf_i.push_back(a); pf_j.push_back(b); pf_l.push_back(l);
            const double p6[6] = {0.1 * l - 0.3, 0.05 * k, 1.0, 0.1 * l - 0.33, 0.05 * k + 0.01, 1.0};
            pts.insert(pts.end(), p6, p6 + 6);
        }
    const int line_frame[2] = {1, 3};
    const double line_data[18] = {0, 0, 3, 1, 0, 3, 0, 1, -0.1, 0, 1, 3, 1, 1, 3, 0, 1, -0.4};
    tcv_window_desc w = {};
    w.n_frames = F; w.n_landmarks = L; w.n_imu = F - 1; w.n_proj = (int)pf_i.size(); w.n_line = 2;
    w.estimate_extrinsic = 1;
    w.para_pose = &pose[0][0]; w.para_speedbias = &sb[0][0]; w.para_ex_pose = ex; w.para_feature = lam;
    w.imu_frame_i = fi.data(); w.imu_frame_j = fj.data(); w.imu = imu.data();
    w.proj_frame_i = pf_i.data(); w.proj_frame_j = pf_j.data(); w.proj_feature = pf_l.data(); w.proj_pts = pts.data();
    w.proj_sqrt_info = 460.0 / 1.5; w.proj_loss_a = 1.0;
    w.line_frame = line_frame; w.line_data = line_data;
    const double K[9] = {460, 0, 376, 0, 460, 240, 0, 0, 1}, I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::copy(K, K + 9, w.line_K); std::copy(I3, I3 + 9, w.line_Ric);
    w.line_loss_a = 1.0; w.gravity[2] = 9.8; w.td_ROW = 1.0;
    tcv_problem *p = nullptr;
    CHECK(tcv_problem_from_window(&w, &p) == TCV_OK);
    std::vector<double *> fp, fs;
    for (int i = 0; i < F; i++) { fp.push_back(pose[i]); fs.push_back(sb[i]); }
    CHECK(tcv_problem_set_frames(p, F, fp.data(), fs.data()) == TCV_OK);

    for (int mode = 0; mode < 2; mode++) {
        Packed pk;
        CHECK(pack_problem(*p, pk, nullptr, mode) == TCV_OK);
        const PlanHdr &H = pk.hdr;
        CHECK(H.nland == L && H.n_proj == w.n_proj && H.n_imu == F - 1 && H.n_line == 2);
        std::vector<int> lists;
        int jd = 0;
        CHECK(cov_owner_lists(*p, pk, H, lists, &jd) == TCV_OK);
        CHECK((int)lists.size() > CT_HDR && lists[CT_JDOUBLES] == jd && lists[CT_NPAIR] > 0 && lists[CT_OPAIR] == CT_HDR);
        CHECK(lists[CT_OLMFAC] + H.n_proj == (int)lists.size());      // the last array: one entry per point factor
        const int *lmptr = lists.data() + lists[CT_OLMPTR];
        CHECK(lmptr[0] == 0 && lmptr[L] == H.n_proj);
        for (int k = 0; k < lists[CT_NPAIR]; k++) {      // every item offset of every pair lies inside the J region
            const int *pr = lists.data() + lists[CT_OPAIR] + CT_PAIR * k;
            CHECK(pr[0] >= pr[1] && pr[0] + pr[2] <= H.nc && pr[4] <= pr[5]);
            for (int it = pr[4]; it < pr[5]; it++) {
                const int *q = lists.data() + lists[CT_OITEM] + CT_ITEM * it;
                CHECK(q[0] >= 0 && q[0] < jd && q[1] >= 0 && q[1] < jd && q[3] < jd);
            }
        }
        const CovLmSlots S = cov_landmark_slots(*p, pk, H);
        CHECK(S.jdoubles == jd && (int)S.sptr.size() == L + 1 && S.blk.size() == S.off.size() && S.blk.size() == S.items.size());
        CHECK(lists[CT_NHSLOT] == (int)S.blk.size());
        const std::vector<int> lt = cov_slot_table(*p, pk, S);
        CHECK((int)lt.size() == L + 1 + LT_SLOT * (int)S.blk.size() && lt[0] == 0 && lt[L] == (int)S.blk.size());
        for (int l = 0; l < L; l++)
            for (int s = lt[l]; s < lt[l + 1]; s++) {
                const int *r = lt.data() + L + 1 + LT_SLOT * s;
                CHECK(r[0] >= 0 && r[0] + r[2] <= H.nc && r[1] + COV_SLOT <= jd);
                if (s > lt[l]) CHECK(r[0] > r[-LT_SLOT]);      // ascending tangent order
            }
        // request tables of a one-window batch (nothing but the host maps of the batch is read)
        tcv_batch b;
        b.in.n = 1; b.in.problems.push_back(p); b.in.packed.push_back(pk); b.in.plans.push_back(H); b.in.wins.push_back(pk.win);
        const tcv_covariance_block rq[4] = {{TCV_COV_POSE, -1, TCV_COV_POSE, -1}, {TCV_COV_POSE, -1, TCV_COV_SPEED_BIAS, -1}, {TCV_COV_EXTRINSIC, 0, TCV_COV_POSE, 0},
                                            {TCV_COV_SPEED_BIAS, 1, TCV_COV_SPEED_BIAS, 1}};
        std::vector<int> tab, rows, cols;
        CHECK(cov_request_tables(&b, rq, 4, tab, rows, cols) == TCV_OK);
        CHECK((int)tab.size() == cov_rq_stride(4) && tab[RQ_NREQ] == 4 && tab[RQ_M] == 6 + 9 + 6 + 6 + 9 && rows[1] == 6 && cols[1] == 9);
        for (int c = 0; c < tab[RQ_M]; c++) CHECK(tab[RQ_COL + c] >= 0 && tab[RQ_COL + c] < H.nc);
        const tcv_covariance_block bad[1] = {{TCV_COV_TD, 0, TCV_COV_TD, 0}};
        CHECK(cov_request_tables(&b, bad, 1, tab, rows, cols) == TCV_ERR_INVALID);
        int blk = -1, width = 0;
        CHECK(cov_resolve(*p, TCV_COV_LANDMARK, 0, &blk, &width) == TCV_ERR_UNSUPPORTED && cov_resolve(*p, TCV_COV_POSE, F, &blk, &width) == TCV_ERR_INVALID);
        std::printf("mode %d: nc %d, %d pairs, %d owner-list ints, %d slots, %d slot-table ints, J region %d doubles\n", mode, H.nc, lists[CT_NPAIR], (int)lists.size(),
                    (int)S.blk.size(), (int)lt.size(), jd);
    }
    tcv_problem_destroy(p);
    std::printf("ok\n");
    return 0;
}
