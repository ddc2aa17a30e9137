// C-ABI of include/tcv.h, host only: the ceres::Problem-shaped graph building, tcv_problem_from_window, the packer's diagnostics
// (plan statistics, marginalisation plan, packing benchmark, plan cache) and the MarginalizationInfo-shaped prior handles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "tcv_host.h"

using namespace tcv;

// =====================================================================================================
// ceres::Problem surface
// =====================================================================================================
extern "C" int tcv_problem_create(tcv_problem **out) {
    if (!out) return TCV_ERR_INVALID;
    *out = new tcv_problem();
    return TCV_OK;
}
extern "C" void tcv_problem_destroy(tcv_problem *p) { delete p; }

static int block_of(tcv_problem *p, double *addr) {
    return p->index.find(addr);
}

extern "C" int tcv_problem_add_parameter_block(tcv_problem *p, double *values, int size, int parameterization) {
    if (!p || !values || size <= 0) { set_error("add_parameter_block: bad argument"); return TCV_ERR_INVALID; }
    if (parameterization == TCV_PARAM_POSE && size != 7) { set_error("pose parameterisation needs a size-7 block"); return TCV_ERR_INVALID; }
    const int b = block_of(p, values);
    if (b >= 0) {  // Ceres 2.x accepts re-adding a block (estimator.cpp:1837-1838); size must agree
        if (p->blocks[b].size != size) { set_error("parameter block re-added with a different size"); return TCV_ERR_INVALID; }
        p->blocks[b].kind = parameterization == TCV_PARAM_POSE ? KIND_POSE : p->blocks[b].kind;
        return TCV_OK;
    }
    p->index.put(values, (int)p->blocks.size());
    p->blocks.push_back(ParamBlock{values, size, parameterization == TCV_PARAM_POSE ? KIND_POSE : KIND_EUCLID, false});
    return TCV_OK;
}
extern "C" int tcv_problem_set_parameter_block_constant(tcv_problem *p, double *values) {
    const int b = p ? block_of(p, values) : -1;
    if (b < 0) { set_error("set_parameter_block_constant: unknown block"); return TCV_ERR_INVALID; }
    p->blocks[b].constant = true;
    return TCV_OK;
}
extern "C" int tcv_problem_set_gravity(tcv_problem *p, const double G[3]) {
    if (!p || !G) return TCV_ERR_INVALID;
    for (int i = 0; i < 3; i++) p->G[i] = G[i];
    return TCV_OK;
}
// implicit AddParameterBlock like ceres::Problem::AddResidualBlock does for unknown pointers
static int ensure_block(tcv_problem *p, double *addr, int size) {
    int b = block_of(p, addr);
    if (b >= 0) return p->blocks[b].size == size ? b : -1;
    if (tcv_problem_add_parameter_block(p, addr, size, TCV_PARAM_EUCLIDEAN) != TCV_OK) return -1;
    return block_of(p, addr);
}
// the four parameter blocks of a factor (added when unknown); false: a NULL address or a block of another size
static bool bind_blocks(tcv_problem *p, double *const a[4], const int sz[4], int b[4]) {
    for (int k = 0; k < 4; k++) if ((b[k] = a[k] ? ensure_block(p, a[k], sz[k]) : -1) < 0) return false;
    return true;
}
extern "C" int tcv_problem_add_imu_factor(tcv_problem *p, const tcv_imu_preintegration *pre, double *pose_i, double *sb_i,
                                          double *pose_j, double *sb_j) {
    if (!p || !pre) return TCV_ERR_INVALID;
    ImuFac f;
    f.pre = *pre;
    double *a[4] = {pose_i, sb_i, pose_j, sb_j};
    const int sz[4] = {7, 9, 7, 9};
    if (!bind_blocks(p, a, sz, f.b)) { set_error("add_imu_factor: bad parameter block"); return TCV_ERR_INVALID; }
    p->imu.push_back(f);
    return TCV_OK;
}
extern "C" int tcv_problem_add_imu_factor_device(tcv_problem *p, const tcv_preint *pre, double *pose_i, double *sb_i, double *pose_j, double *sb_j) {
    if (!p || !pre) return TCV_ERR_INVALID;
    ImuFac f;
    std::memset(&f.pre, 0, sizeof f.pre);
    f.pre.sum_dt = pre->sum_dt;
    f.dev = pre;
    double *a[4] = {pose_i, sb_i, pose_j, sb_j};
    const int sz[4] = {7, 9, 7, 9};
    if (!bind_blocks(p, a, sz, f.b)) { set_error("add_imu_factor_device: bad parameter block"); return TCV_ERR_INVALID; }
    p->imu.push_back(f);
    return TCV_OK;
}
extern "C" int tcv_problem_add_projection_factor(tcv_problem *p, const double pts_i[3], const double pts_j[3], double sqrt_info,
                                                 double loss_a, double *pose_i, double *pose_j, double *ex_pose,
                                                 double *inv_depth) {
    if (!p || !pts_i || !pts_j) return TCV_ERR_INVALID;
    ProjFac f;
    for (int i = 0; i < 3; i++) { f.pts[i] = pts_i[i]; f.pts[3 + i] = pts_j[i]; }
    f.sqrt_info = sqrt_info; f.loss_a = loss_a;
    double *a[4] = {pose_i, pose_j, ex_pose, inv_depth};
    const int sz[4] = {7, 7, 7, 1};
    if (!bind_blocks(p, a, sz, f.b)) { set_error("add_projection_factor: bad parameter block"); return TCV_ERR_INVALID; }
    for (int i = 0; i < 8; i++) f.aux[i] = 0.0;
    f.btd = -1;
    p->proj.push_back(f);
    return TCV_OK;
}
extern "C" int tcv_problem_add_projection_td_factor(tcv_problem *p, const double pts_i[3], const double pts_j[3], const double vel_i[2],
                                                    const double vel_j[2], double td_i, double td_j, double row_i, double row_j, double sqrt_info,
                                                    double loss_a, double *pose_i, double *pose_j, double *ex_pose, double *inv_depth, double *td) {
    if (!p || !vel_i || !vel_j || !td) { set_error("add_projection_td_factor: bad argument"); return TCV_ERR_INVALID; }
    const int btd = ensure_block(p, td, 1);
    if (btd < 0) { set_error("add_projection_td_factor: bad td block"); return TCV_ERR_INVALID; }
    const int rc = tcv_problem_add_projection_factor(p, pts_i, pts_j, sqrt_info, loss_a, pose_i, pose_j, ex_pose, inv_depth);
    if (rc != TCV_OK) return rc;
    ProjFac &f = p->proj.back();
    f.aux[0] = vel_i[0]; f.aux[1] = vel_i[1]; f.aux[2] = vel_j[0]; f.aux[3] = vel_j[1];
    f.aux[4] = td_i; f.aux[5] = td_j; f.aux[6] = row_i; f.aux[7] = row_j;
    f.btd = btd;
    return TCV_OK;
}
extern "C" int tcv_problem_set_line_jacobian(tcv_problem *p, int exact) {
    if (!p || (exact != 0 && exact != 1)) { set_error("set_line_jacobian: 0 (reference) or 1 (exact)"); return TCV_ERR_INVALID; }
    p->line_exact = exact;
    return TCV_OK;
}
extern "C" int tcv_problem_set_rolling_shutter(tcv_problem *p, double TR, double ROW) {
    if (!p || !(ROW > 0.0) || !(TR == TR)) { set_error("set_rolling_shutter: ROW must be positive"); return TCV_ERR_INVALID; }
    p->td_TR = TR; p->td_ROW = ROW;
    return TCV_OK;
}
extern "C" int tcv_problem_add_line_factor(tcv_problem *p, const double ps[3], const double pe[3], const double abc[3],
                                           const double K[9], const double R[9], const double T[3], double loss_a, double *pose) {
    if (!p || !ps || !pe || !abc || !K || !R || !T || !pose) return TCV_ERR_INVALID;
    LineFac f;
    for (int i = 0; i < 3; i++) { f.d[i] = ps[i]; f.d[3 + i] = pe[i]; f.d[6 + i] = abc[i]; f.T[i] = T[i]; }
    for (int i = 0; i < 9; i++) { f.K[i] = K[i]; f.R[i] = R[i]; }
    f.loss_a = loss_a;
    f.b = ensure_block(p, pose, 7);
    if (f.b < 0) { set_error("add_line_factor: bad parameter block"); return TCV_ERR_INVALID; }
    p->line.push_back(f);
    return TCV_OK;
}
extern "C" int tcv_problem_add_marginalization_factor(tcv_problem *p, const tcv_prior *prior, double *const *blocks, int n) {
    if (!p || !prior || n != (int)prior->size.size() || (n > 0 && !blocks)) { set_error("add_marginalization_factor: block count mismatch"); return TCV_ERR_INVALID; }
    // the prior of a marginalisation that kept nothing (n = 0): the reference adds a MarginalizationFactor with no residuals over no blocks
    // (estimator.cpp:1714-1720 on the empty MarginalizationInfo of marginalization_factor.cpp:174-194) -- accepted, contributes nothing
    if (prior->n == 0) return TCV_OK;
    PriorFac f;
    f.prior = prior;
    for (int k = 0; k < n; k++) {
        const int b = ensure_block(p, blocks[k], prior->size[k]);
        if (b < 0) { set_error("add_marginalization_factor: bad parameter block"); return TCV_ERR_INVALID; }
        f.b.push_back(b);
    }
    p->prior.push_back(f);
    return TCV_OK;
}
extern "C" int tcv_problem_set_frames(tcv_problem *p, int n_frames, double *const *pose, double *const *speedbias) {
    if (!p || n_frames <= 0 || !pose) { set_error("set_frames: bad argument"); return TCV_ERR_INVALID; }
    std::vector<int> fp(n_frames, -1), fs(n_frames, -1);
    for (int i = 0; i < n_frames; i++) {
        fp[i] = block_of(p, pose[i]);
        if (fp[i] < 0 || p->blocks[fp[i]].size != 7) { set_error("set_frames: unknown pose block"); return TCV_ERR_INVALID; }
        if (speedbias && speedbias[i]) {
            fs[i] = block_of(p, speedbias[i]);
            if (fs[i] < 0 || p->blocks[fs[i]].size != 9) { set_error("set_frames: unknown speed-bias block"); return TCV_ERR_INVALID; }
        }
    }
    p->frame_pose = fp; p->frame_sb = fs;
    return TCV_OK;
}
// relo_Pose of estimator.cpp:1854-1886 and what double2vector's tail (:1606-1624) needs besides the solved states: relo_frame_local_index,
// prev_relo_t / prev_relo_r.  The block itself and its ProjectionFactors were added before (tcv_problem_add_parameter_block / _projection_factor).
extern "C" int tcv_problem_set_relocalization(tcv_problem *p, double *relo_pose, int frame_local_index, const double prev_relo_t[3], const double prev_relo_r[9]) {
    if (!p || !prev_relo_t || !prev_relo_r) { set_error("set_relocalization: bad argument"); return TCV_ERR_INVALID; }
    const int b = block_of(p, relo_pose);
    if (b < 0 || p->blocks[b].size != 7 || p->blocks[b].kind != KIND_POSE) { set_error("set_relocalization: relo_pose is not a pose block (size 7, TCV_PARAM_POSE) of the problem"); return TCV_ERR_INVALID; }
    if (p->frame_pose.empty()) { set_error("set_relocalization: the problem carries no frame table (tcv_problem_set_frames)"); return TCV_ERR_INVALID; }
    for (int f : p->frame_pose) if (f == b) { set_error("set_relocalization: relo_pose is one of the frame poses"); return TCV_ERR_INVALID; }
    if (frame_local_index < 0 || frame_local_index >= (int)p->frame_pose.size()) { set_error("set_relocalization: frame_local_index outside [0, n_frames)"); return TCV_ERR_INVALID; }
    for (int i = 0; i < 12; i++) if (!std::isfinite(i < 3 ? prev_relo_t[i] : prev_relo_r[i - 3])) { set_error("set_relocalization: prev_relo_t / prev_relo_r not finite"); return TCV_ERR_INVALID; }
    p->relo_block = b; p->relo_local = frame_local_index;
    std::memcpy(p->relo_prev, prev_relo_t, 24); std::memcpy(p->relo_prev + 3, prev_relo_r, 72);
    return TCV_OK;
}
extern "C" int tcv_problem_num_parameter_blocks(const tcv_problem *p) { return p ? (int)p->blocks.size() : 0; }
extern "C" int tcv_problem_num_residual_blocks(const tcv_problem *p) {
    return p ? (int)(p->imu.size() + p->proj.size() + p->line.size() + p->prior.size()) : 0;
}
extern "C" int tcv_problem_num_residuals(const tcv_problem *p) {
    if (!p) return 0;
    int n = 15 * (int)p->imu.size() + 2 * (int)p->proj.size() + 2 * (int)p->line.size();
    for (auto &f : p->prior) n += f.prior->n;
    return n;
}

// host-only: packs the problem (no device needed) and reports the sizes of its plan and data.
// out[0..15] = nc, nx, npp, nland, nt, n_vis_chunk, n_imu_chunk, n_vunit, n_vitem, n_sunit, n_sitem, n_iunit, n_iitem,
//              plan ints, window doubles, LDS bytes
extern "C" int tcv_problem_plan_stats(const tcv_problem *p, int *out) {
    if (!p || !out) return TCV_ERR_INVALID;
    Packed pk;
    const char *ec = getenv("TCV_PLAN_COOP");      // developer / test switch: the plan the cooperative mode would use with that many helpers
    const int rc = pack_problem(*p, pk, nullptr, solver_variant(), 0, false, ec ? atoi(ec) : 0);
    if (rc != TCV_OK) return rc;
    const PlanHdr &H = pk.hdr;
    const int v[16] = {H.nc, H.nx, H.npp, H.nland, H.chain ? H.nt_c : H.nt, H.n_vis_chunk, H.n_imu_chunk, H.n_vunit, H.n_vitem, H.n_sunit, H.n_sitem,
                       H.chain ? H.n_e : H.n_iunit, H.n_iitem, H.plan_ints, pk.win.n_doubles,
                       H.chain ? chain_lds_doubles() * 8
                               : (H.nt * (H.nt + 1) / 2 * 256 + 2 * ((H.nx + H.nland + 1) & ~1) + (3 * H.camw + 176) + 64 + H.lds_area) * 8};
    std::memcpy(out, v, sizeof v);
    return TCV_OK;
}

// diagnostics of the packer (tests/test_pack_cpu.py): the plan of a problem as the device would get it -- header (as ints) followed by the
// int pool -- and the switch between the fast gather-program builder with its caches and the generic reference builder
extern "C" int tcv_problem_plan_ints(const tcv_problem *p, int *out, int cap, int *len) {
    if (!p || !len) return TCV_ERR_INVALID;
    Packed pk;
    const char *ec = getenv("TCV_PLAN_COOP");
    const int rc = pack_problem(*p, pk, nullptr, solver_variant(), 0, true, ec ? atoi(ec) : 0);
    if (rc != TCV_OK) return rc;
    const PlanInts &pints = pk.tmpl ? pk.tmpl->ints : pk.ints;
    const int nh = (int)(sizeof(PlanHdr) / sizeof(int));
    *len = nh + (int)pints.size();
    if (out && cap >= *len) { std::memcpy(out, &pk.hdr, sizeof(PlanHdr)); std::memcpy(out + nh, pints.data(), sizeof(int) * pints.size()); }
    return TCV_OK;
}
// the same for the marginalisation packer (tests/test_marg_pack_cpu.py): [MargHdr as ints | int pool] and the double pool of one window
extern "C" int tcv_problem_marg_plan(const tcv_problem *mp, double *const *drop, int num_drop, const tcv_problem *solve_p,
                                     int *ints, int ints_cap, int *ints_len, double *doubles, int doubles_cap, int *doubles_len) {
    if (!mp || !ints_len || !doubles_len || num_drop < 0 || (num_drop > 0 && !drop)) return TCV_ERR_INVALID;
    Packed pk;
    if (solve_p) {
        const char *ec = getenv("TCV_PLAN_COOP");
        if (const int rc = pack_problem(*solve_p, pk, nullptr, solver_variant(), 0, true, ec ? atoi(ec) : 0)) return rc;
    }
    std::vector<int> I;
    std::vector<double> D;
    if (const int rc = tcv_marg_plan(*mp, drop, num_drop, solve_p, solve_p ? &pk : nullptr, I, D)) return rc;
    *ints_len = (int)I.size(); *doubles_len = (int)D.size();
    if (ints && ints_cap >= *ints_len && !I.empty()) std::memcpy(ints, I.data(), sizeof(int) * I.size());
    if (doubles && doubles_cap >= *doubles_len && !D.empty()) std::memcpy(doubles, D.data(), sizeof(double) * D.size());
    return TCV_OK;
}
extern "C" int tcv_set_packer_reference(int on) { tcv::set_pack_reference(on); return TCV_OK; }
// the packing pass of tcv_batch_create (plans + data sizes of n problems on `threads` host threads of the library's worker pool) without
// a device: seconds of wall time in *seconds
extern "C" int tcv_problems_pack_bench(tcv_problem *const *problems, int n, int threads, int coop_chunks, double *seconds) {
    if (!problems || n <= 0 || !seconds) return TCV_ERR_INVALID;
    // TCV_PACK_BENCH_FRAME = f: the problems are packed f at a time and every group's plans are released before the next group starts --
    // the life cycle of a lock-step frame's batch (the int pools come back from the block pool) instead of n plans alive at once
    int frame = n;
    if (const char *e = getenv("TCV_PACK_BENCH_FRAME")) { const int v = atoi(e); if (v > 0) frame = std::min(n, v); }
    PackErrors err(n, n);      // (the text is per thread: a worker's is carried over to the caller below)
    const auto t0 = std::chrono::steady_clock::now();
    for (int b = 0; b < n; b += frame) {
        const int m = std::min(frame, n - b), nth = std::max(1, std::min(threads, m));
        std::vector<Packed> packed(m);
        tcv::parallel_items(m, nth, [&](int w, int) {
            err.note(b + w, b + w, pack_problem(*problems[b + w], packed[w], nullptr, solver_variant(), coop_chunks > 0 ? (int)LDS_DOUBLES : 0, true, coop_chunks));
        });
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (getenv("TCV_DEBUG_PACK2")) tcv::pack_laps_print();
    return err.first();
}
extern "C" int tcv_plan_cache_stats(long long *out4) {
    if (!out4) return TCV_ERR_INVALID;
    long long e = 0;
    tcv::plan_cache_stats(&out4[0], &out4[1], &e);
    tcv::cam_cache_stats(&out4[2], &out4[3]);
    return TCV_OK;
}

// graph construction of estimator.cpp:1683-1846 from frame-indexed arrays
extern "C" int tcv_problem_from_window(const tcv_window_desc *w, tcv_problem **out) {
    if (!w || !out || w->n_frames <= 0 || !w->para_pose || !w->para_speedbias || !w->para_ex_pose || (w->n_imu > 0 && (!w->imu || !w->imu_frame_i || !w->imu_frame_j)) ||
        (w->n_proj > 0 && (!w->proj_pts || !w->proj_frame_i || !w->proj_frame_j || !w->proj_feature || !w->para_feature)) ||
        (w->n_line > 0 && (!w->line_data || !w->line_frame)) ||
        (w->prior && w->prior->n > 0 && (!w->prior_block_kind || !w->prior_block_index)) || w->n_imu < 0 || w->n_proj < 0 || w->n_line < 0 ||
        (w->para_td && w->n_proj > 0 && !w->proj_td_aux) || (w->para_td && !(w->td_ROW > 0.0))) {
        set_error("problem_from_window: missing array in the window description");
        return TCV_ERR_INVALID;
    }
    auto frame_ok = [&](int f) { return f >= 0 && f < w->n_frames; };
    for (int k = 0; k < w->n_imu; k++) if (!frame_ok(w->imu_frame_i[k]) || !frame_ok(w->imu_frame_j[k])) { set_error("problem_from_window: IMU frame index out of range"); return TCV_ERR_INVALID; }
    for (int k = 0; k < w->n_proj; k++)
        if (!frame_ok(w->proj_frame_i[k]) || !frame_ok(w->proj_frame_j[k]) || w->proj_feature[k] < 0 || w->proj_feature[k] >= w->n_landmarks) { set_error("problem_from_window: projection frame / feature index out of range"); return TCV_ERR_INVALID; }
    for (int k = 0; k < w->n_line; k++) if (!frame_ok(w->line_frame[k])) { set_error("problem_from_window: line frame index out of range"); return TCV_ERR_INVALID; }
    tcv_problem *p = new tcv_problem();
    int rc = TCV_OK;
    auto chk = [&](int r) { if (rc == TCV_OK && r != TCV_OK) rc = r; };
    for (int i = 0; i < w->n_frames; i++) {   // :1683-1688
        chk(tcv_problem_add_parameter_block(p, w->para_pose + 7 * i, 7, TCV_PARAM_POSE));
        chk(tcv_problem_add_parameter_block(p, w->para_speedbias + 9 * i, 9, TCV_PARAM_EUCLIDEAN));
    }
    chk(tcv_problem_add_parameter_block(p, w->para_ex_pose, 7, TCV_PARAM_POSE));   // :1689-1701
    if (!w->estimate_extrinsic) chk(tcv_problem_set_parameter_block_constant(p, w->para_ex_pose));
    chk(tcv_problem_set_gravity(p, w->gravity));
    if (w->line_exact_jacobian) chk(tcv_problem_set_line_jacobian(p, 1));
    if (w->para_td) {   // :1703-1707
        chk(tcv_problem_add_parameter_block(p, w->para_td, 1, TCV_PARAM_EUCLIDEAN));
        chk(tcv_problem_set_rolling_shutter(p, w->td_TR, w->td_ROW));
    }
    if (w->prior) {   // :1714-1720
        int m, n, nb, xs;
        tcv_prior_dims(w->prior, &m, &n, &nb, &xs);
        std::vector<double *> blocks(nb);
        for (int k = 0; k < nb; k++) {
            const int kind = w->prior_block_kind[k], idx = w->prior_block_index[k];
            if (kind < 0 || kind > 3 || (kind < 2 && !frame_ok(idx)) || (kind == 3 && !w->para_td)) { set_error("problem_from_window: prior block kind / index out of range"); rc = TCV_ERR_INVALID; break; }
            blocks[k] = kind == 0 ? w->para_pose + 7 * idx : (kind == 1 ? w->para_speedbias + 9 * idx : (kind == 2 ? w->para_ex_pose : w->para_td));
        }
        if (rc == TCV_OK) chk(tcv_problem_add_marginalization_factor(p, w->prior, blocks.data(), nb));
    }
    for (int k = 0; k < w->n_imu; k++) {   // :1723-1732
        if (w->imu[k].sum_dt > 10.0) continue;
        const int i = w->imu_frame_i[k], j = w->imu_frame_j[k];
        if (w->imu_device && w->imu_device[k])
            chk(tcv_problem_add_imu_factor_device(p, w->imu_device[k], w->para_pose + 7 * i, w->para_speedbias + 9 * i, w->para_pose + 7 * j,
                                                  w->para_speedbias + 9 * j));
        else
        chk(tcv_problem_add_imu_factor(p, w->imu + k, w->para_pose + 7 * i, w->para_speedbias + 9 * i, w->para_pose + 7 * j,
                                       w->para_speedbias + 9 * j));
    }
    // The point and line factors: same result as tcv_problem_add_projection[_td]_factor / tcv_problem_add_line_factor per factor (blocks the
    // factors introduce are added in order of first appearance, like ceres::Problem::AddResidualBlock does for unknown pointers), but the
    // block indices of the frame-indexed arrays are known here -- no address lookup per pointer (four per point factor: a third of a
    // lock-step frame's problem construction)
    if (rc == TCV_OK) {
        const int b_ex = block_of(p, w->para_ex_pose), b_td = w->para_td ? block_of(p, w->para_td) : -1;
        std::vector<int> b_pose(w->n_frames), b_feat(std::max(1, w->n_landmarks), -1);
        for (int i = 0; i < w->n_frames; i++) b_pose[i] = block_of(p, w->para_pose + 7 * i);
        p->proj.reserve((size_t)w->n_proj); p->line.reserve((size_t)w->n_line);
        p->blocks.reserve(p->blocks.size() + (size_t)w->n_landmarks);
        for (int k = 0; k < w->n_proj && rc == TCV_OK; k++) {   // :1737-1771
            const int l = w->proj_feature[k];
            if (b_feat[l] < 0) {
                double *addr = w->para_feature + l;
                b_feat[l] = ensure_block(p, addr, 1);      // (an address that is a block already must be a size-1 block)
                if (b_feat[l] < 0) { set_error("add_projection_factor: bad parameter block"); rc = TCV_ERR_INVALID; break; }
            }
            p->proj.emplace_back();
            ProjFac &f = p->proj.back();
            const double *pt = w->proj_pts + 6 * k;
            for (int i = 0; i < 6; i++) f.pts[i] = pt[i];
            f.sqrt_info = w->proj_sqrt_info; f.loss_a = w->proj_loss_a;
            f.b[0] = b_pose[w->proj_frame_i[k]]; f.b[1] = b_pose[w->proj_frame_j[k]]; f.b[2] = b_ex; f.b[3] = b_feat[l];
            if (w->para_td) { const double *a = w->proj_td_aux + 8 * k; for (int i = 0; i < 8; i++) f.aux[i] = a[i]; f.btd = b_td; }
            else { for (int i = 0; i < 8; i++) f.aux[i] = 0.0; f.btd = -1; }
        }
        for (int k = 0; k < w->n_line && rc == TCV_OK; k++) {   // :1786-1846
            p->line.emplace_back();
            LineFac &f = p->line.back();
            const double *d = w->line_data + 9 * k;
            for (int i = 0; i < 9; i++) { f.d[i] = d[i]; f.K[i] = w->line_K[i]; f.R[i] = w->line_Ric[i]; }
            for (int i = 0; i < 3; i++) f.T[i] = w->line_Tic[i];
            f.loss_a = w->line_loss_a;
            f.b = b_pose[w->line_frame[k]];
        }
    }
    {
        std::vector<double *> fp(w->n_frames), fs(w->n_frames);
        for (int i = 0; i < w->n_frames; i++) { fp[i] = w->para_pose + 7 * i; fs[i] = w->para_speedbias + 9 * i; }
        chk(tcv_problem_set_frames(p, w->n_frames, fp.data(), fs.data()));
    }
    if (rc != TCV_OK) { delete p; return rc; }
    *out = p;
    return TCV_OK;
}

// =====================================================================================================
// prior (MarginalizationInfo layout, marginalization_factor.h:57-70)
// =====================================================================================================
extern "C" int tcv_prior_create(tcv_prior **out, int m, int n, int nb, const int *size, const int *idx, const double *x0,
                                const double *J0, const double *r0) {
    if (out && n == 0 && nb == 0 && m >= 0) {      // the empty MarginalizationInfo of a marginalisation that kept nothing (tcv_marginalize can return one)
        tcv_prior *pr = new tcv_prior();
        pr->m = m;
        *out = pr;
        return TCV_OK;
    }
    if (!out || n <= 0 || nb <= 0 || m < 0 || !size || !idx || !x0 || !J0 || !r0) { set_error("prior_create: bad argument"); return TCV_ERR_INVALID; }
    // the kernels index fixed-size (128-entry) dx / residual buffers by keep_block_idx: a malformed layout must not reach the device
    if (n > 128) { set_error("prior_create: more than 128 rows"); return TCV_ERR_TOO_LARGE; }
    {
        std::vector<char> used(n, 0);
        int sum_local = 0;
        for (int k = 0; k < nb; k++) {
            if (size[k] <= 0) { set_error("prior_create: keep_block_size must be positive"); return TCV_ERR_INVALID; }
            const int local = size[k] == 7 ? 6 : size[k];      // MarginalizationInfo::localSize, marginalization_factor.cpp:100-103
            if (idx[k] < m || idx[k] - m + local > n) { set_error("prior_create: keep_block_idx outside [m, m + n)"); return TCV_ERR_INVALID; }
            for (int j = 0; j < local; j++) {
                if (used[idx[k] - m + j]) { set_error("prior_create: kept blocks overlap"); return TCV_ERR_INVALID; }
                used[idx[k] - m + j] = 1;
            }
            sum_local += local;
        }
        if (sum_local != n) { set_error("prior_create: local sizes of the kept blocks do not sum to n"); return TCV_ERR_INVALID; }
    }
    tcv_prior *pr = new tcv_prior();
    pr->m = m; pr->n = n;
    int xs = 0;
    for (int k = 0; k < nb; k++) {   // keep_block_idx counts from the start of the [m | n] ordering (marginalization_factor.cpp:312, :347)
        pr->size.push_back(size[k]); pr->idx.push_back(idx[k] - m); pr->xoff.push_back(xs); xs += size[k];
    }
    pr->x0.assign(x0, x0 + xs);
    pr->xsize = xs;
    pr->J0.assign(J0, J0 + (size_t)n * n);
    pr->r0.assign(r0, r0 + n);
    pr->addr.assign(nb, nullptr);
    *out = pr;
    return TCV_OK;
}
extern "C" int tcv_prior_dims(const tcv_prior *pr, int *m, int *n, int *nb, int *xs) {
    if (!pr) return TCV_ERR_INVALID;
    if (m) *m = pr->m;
    if (n) *n = pr->n;
    if (nb) *nb = (int)pr->size.size();
    if (xs) *xs = pr->xsize;
    return TCV_OK;
}
extern "C" int tcv_prior_is_device_resident(const tcv_prior *pr) {
    if (!pr) return 0;
    std::lock_guard<std::mutex> g(pr->mu);
    return pr->host ? 0 : 1;
}
extern "C" int tcv_prior_export(const tcv_prior *pr, int *size, int *idx, double *x0, double *J0, double *r0) {
    if (!pr) return TCV_ERR_INVALID;
    if (x0 || J0 || r0) if (int rc = tcv_prior_host(pr)) return rc;      // a device-resident prior is materialised on demand
    if (size) std::copy(pr->size.begin(), pr->size.end(), size);
    if (idx) for (size_t k = 0; k < pr->idx.size(); k++) idx[k] = pr->idx[k] + pr->m;
    if (x0) std::copy(pr->x0.begin(), pr->x0.end(), x0);
    if (J0) std::copy(pr->J0.begin(), pr->J0.end(), J0);
    if (r0) std::copy(pr->r0.begin(), pr->r0.end(), r0);
    return TCV_OK;
}
// parity/debug: the Schur system (A' n x n row-major, b') the prior was factored from; TCV_ERR_INVALID if not recorded
extern "C" int tcv_prior_export_schur(const tcv_prior *pr, double *As, double *bs) {
    if (pr && pr->n == 0) return TCV_OK;      // (the empty prior of a marginalisation that kept nothing: nothing to copy)
    if (!pr || pr->As.empty()) { set_error("prior carries no Schur system"); return TCV_ERR_INVALID; }
    if (As) std::copy(pr->As.begin(), pr->As.end(), As);
    if (bs) std::copy(pr->bs.begin(), pr->bs.end(), bs);
    return TCV_OK;
}
extern "C" int tcv_prior_keep_block_addresses(const tcv_prior *pr, double **addresses) {
    if (!pr || !addresses) return TCV_ERR_INVALID;
    std::copy(pr->addr.begin(), pr->addr.end(), addresses);
    return TCV_OK;
}
extern "C" void tcv_prior_destroy(tcv_prior *pr) { delete pr; }
extern "C" int tcv_problem_set_marginalization_prior(tcv_problem *p, const tcv_prior *prior) {
    if (!p || !prior || p->prior.size() != 1) { set_error("set_marginalization_prior: the problem must hold exactly one marginalisation factor"); return TCV_ERR_INVALID; }
    const tcv_prior *old = p->prior[0].prior;
    if (old->n != prior->n || old->size != prior->size || old->idx != prior->idx) { set_error("set_marginalization_prior: the new prior has another layout"); return TCV_ERR_INVALID; }
    p->prior[0].prior = prior;
    return TCV_OK;
}
extern "C" int tcv_problems_set_marginalization_prior(tcv_problem *const *problems, tcv_prior *const *priors, int n) {
    if (!problems || !priors || n < 0) return TCV_ERR_INVALID;
    for (int k = 0; k < n; k++) if (int rc = tcv_problem_set_marginalization_prior(problems[k], priors[k])) return rc;
    return TCV_OK;
}
extern "C" void tcv_priors_destroy(tcv_prior *const *priors, int n) {
    if (priors) for (int k = 0; k < n; k++) delete priors[k];
}
