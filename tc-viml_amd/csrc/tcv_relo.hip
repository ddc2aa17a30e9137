// Relocalisation: the tail of Estimator::double2vector() (reference vins_estimator/src/estimator.cpp:1606-1624) on the device.  A window that
// carries relo_Pose (:1854-1886, tcv_problem_set_relocalization) gets one record -- relo_r / relo_t, drift_correct_r / _t, relo_relative_t /
// _q / _yaw (tcv_relo.h) -- computed from the solved, UN-FIXED states right before the gauge fix overwrites pose 0 (tcv_batch_gauge_fix
// launches relo_fix_batch_kernel, then gauge_batch_kernel, on the same stream).  The record travels to the host with the states.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "tcv_host.h"
#include "tcv_math.h"
#include "tcv_relo.h"

namespace tcv {

// n independent cases from host arrays (tcv_relocalization_fix): in = n x [R0 9 | P0 3 | pose0 7 | pose_l 7 | relo_pose 7 | prev 12]
enum { RELO_CASE_IN = 45 };
__global__ void __launch_bounds__(64) relo_fix_kernel(int n, const double *in, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *c = in + (size_t)RELO_CASE_IN * i;
    double rec[RELO_REC];
    relo_tail(m3_load(c), c + 9, c + 12, c + 19, c + 26, c + 33, rec);
    double *o = out + (size_t)RELO_REC * i;
    for (int k = 0; k < RELO_REC; k++) o[k] = rec[k];
}

// batch: one work-item per relocalisation window.  Reads the window header, the initial pose 0 from the data pool and the solved states
// exactly as gauge_batch_kernel does (tcv_gauge.hip), and must run BEFORE it: rot_diff comes from the un-fixed pose 0.
__global__ void __launch_bounds__(64) relo_fix_batch_kernel(int n_relo, const ReloEntry *tab, const double *prev, const WinHdr *win, const PlanHdr *plans,
                                                            const long long *plan_base, const int *ipool, const double *dpool, const double *state,
                                                            int state_stride, double *out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_relo) return;
    const ReloEntry T = tab[e];
    const WinHdr &W = win[T.window];
    const PlanHdr &P = plans[W.plan];
    const int *ft = ipool + plan_base[W.plan] + P.o_frames;
    const double *x = state + (size_t)T.window * state_stride;
    const double *x_init = dpool + W.dbase + W.d_x;
    double rec[RELO_REC];
    for (int k = 0; k < RELO_REC; k++) rec[k] = 0.0;
    const int l = T.local_index;
    if (P.n_frames > 0 && l >= 0 && l < P.n_frames && T.relo_off >= 0 && T.relo_off + 7 <= state_stride) {      // (the host checked all of it: tcv_relo_attach)
        const int g0 = ft[0], gl = ft[2 * l];
        if (g0 >= 0 && gl >= 0) {
            const M3 R0 = to_matrix(Quat(x_init + g0 + 3));      // Rs[0] before the solve: what vector2double() turned into para_Pose[0]
            relo_tail(R0, x_init + g0, x + g0, x + gl, x + T.relo_off, prev + (size_t)RELO_PREV * e, rec);
        }
    }
    double *o = out + (size_t)RELO_REC * e;
    for (int k = 0; k < RELO_REC; k++) o[k] = rec[k];
}

}  // namespace tcv
using namespace tcv;

static void record_to_public(const double *r, int valid, tcv_relo_result *o) {
    static_assert(sizeof(tcv_relo_result) == 8 + sizeof(double) * RELO_REC && offsetof(tcv_relo_result, relo_r) == 8, "tcv_relo_result is two ints and the record");
    o->valid = valid; o->pad_ = 0;
    if (valid) std::memcpy(o->relo_r, r, sizeof(double) * RELO_REC);
    else std::memset(o->relo_r, 0, sizeof(double) * RELO_REC);
}

extern "C" int tcv_relocalization_fix(int n, const double *R0, const double *P0, const double *pose0, const double *pose_l, const double *relo_pose,
                                      const double *prev_relo_t, const double *prev_relo_r, tcv_relo_result *out) {
    if (n <= 0 || n > 4096 || !R0 || !P0 || !pose0 || !pose_l || !relo_pose || !prev_relo_t || !prev_relo_r || !out) { set_error("relocalization_fix: bad argument"); return TCV_ERR_INVALID; }
    if (int rc = device_ready()) return rc;
    const size_t nin = (size_t)RELO_CASE_IN * n, nout = (size_t)RELO_REC * n;
    tcv::RoundTrip rt(tcv::util_stream(), sizeof(double) * nin, sizeof(double) * nout);      // n cases of RELO_CASE_IN doubles -> n records
    if (int rc = rt.ready("relocalization_fix")) return rc;
    double *h = rt.h_in();
    for (int i = 0; i < n; i++) {
        double *c = h + (size_t)RELO_CASE_IN * i;
        std::memcpy(c, R0 + 9 * i, 72); std::memcpy(c + 9, P0 + 3 * i, 24); std::memcpy(c + 12, pose0 + 7 * i, 56); std::memcpy(c + 19, pose_l + 7 * i, 56);
        std::memcpy(c + 26, relo_pose + 7 * i, 56); std::memcpy(c + 33, prev_relo_t + 3 * i, 24); std::memcpy(c + 36, prev_relo_r + 9 * i, 72);
    }
    for (size_t k = 0; k < nin; k++) if (!(h[k] == h[k])) { set_error("relocalization_fix: NaN in the input"); return TCV_ERR_NUMERIC; }
    if (int rc = rt.run("relocalization_fix", [&](hipStream_t st) {
            hipLaunchKernelGGL(relo_fix_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, rt.d_in(), rt.d_out());
        })) return rc;
    for (int i = 0; i < n; i++) record_to_public(rt.h_out() + (size_t)RELO_REC * i, 1, &out[i]);
    return TCV_OK;
}

// tcv_batch_create: the relocalisation table of the batch, its prev_relo_* and the record buffer in one device allocation
// [records RELO_REC x n | prev RELO_PREV x n | table n entries]; the upload goes on `st` (the batch's own upload stream: tcv_batch_create
// waits for it before it returns).  A batch without such a problem allocates, copies and launches nothing.
tcv::ReloState::~ReloState() { tcv::dev_free(d); }
int tcv_relo_attach(tcv_batch *b, hipStream_t st) {
    std::vector<ReloEntry> tab;
    std::vector<double> prev;
    for (int w = 0; w < b->in.n; w++) {
        const tcv_problem &p = *b->in.problems[w];
        if (p.relo_block < 0) continue;
        const Packed &pk = b->in.packed[w];
        const int l = p.relo_local;
        if (l < 0 || l >= (int)p.frame_pose.size() || p.frame_pose.size() > 64) { set_error("batch_create: relocalisation without a frame table (tcv_problem_set_frames)"); return TCV_ERR_INVALID; }
        // where the blocks sit in the state vector: camera blocks in plan order (scatter_states, tcv_batch_results.cpp)
        int off = 0, relo_off = -1;
        bool have0 = false, havel = false;
        for (int blk : pk.cam_block) {
            if (blk == p.relo_block) relo_off = off;
            have0 = have0 || blk == p.frame_pose[0]; havel = havel || blk == p.frame_pose[l];
            off += p.blocks[blk].size;
        }
        if (relo_off < 0 || !have0 || !havel || relo_off + 7 > b->in.state_stride) { set_error("batch_create: the relocalisation pose, para_Pose[0] or the matched frame's pose takes part in no factor"); return TCV_ERR_INVALID; }
        tab.push_back(ReloEntry{w, relo_off, l, 0});
        prev.insert(prev.end(), p.relo_prev, p.relo_prev + RELO_PREV);
    }
    if (tab.empty()) return TCV_OK;
    ReloState *r = new ReloState();
    b->relo.reset(r);
    const size_t nr = tab.size();
    r->n = (int)nr;
    static_assert(sizeof(ReloEntry) == 16, "two doubles per table entry");
    r->win.resize(nr);
    for (size_t k = 0; k < nr; k++) r->win[k] = tab[k].window;
    r->h_up.assign(((size_t)RELO_PREV + 2) * nr, 0.0);
    std::memcpy(r->h_up.data(), prev.data(), sizeof(double) * RELO_PREV * nr);
    std::memcpy(r->h_up.data() + RELO_PREV * nr, tab.data(), sizeof(ReloEntry) * nr);
    hipError_t e = tcv::dev_malloc((void **)&r->d, sizeof(double) * ((size_t)RELO_REC + RELO_PREV + 2) * nr);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    e = hipMemcpyAsync(r->d + RELO_REC * nr, r->h_up.data(), sizeof(double) * r->h_up.size(), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "upload of the relocalisation table");
    return TCV_OK;
}

// tcv_batch_gauge_fix of a batch with relocalisation windows: the records, from the un-fixed states, in front of the gauge kernel
int tcv_relo_launch(tcv_batch *b, hipStream_t st) {
    ReloState *r = tcv_relo_of(b);
    const size_t nr = (size_t)r->n;
    const double *prev = r->d + RELO_REC * nr;
    const ReloEntry *tab = (const ReloEntry *)(prev + RELO_PREV * nr);
    hipLaunchKernelGGL(relo_fix_batch_kernel, dim3((r->n + 63) / 64), dim3(64), 0, st, r->n, tab, prev, b->mem.d_win, b->mem.d_plans, b->mem.d_plan_base, b->mem.d_ipool,
                       b->mem.d_dpool, b->mem.d_state, b->in.state_stride, r->d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "relocalisation kernel launch");
    r->done = true;
    return TCV_OK;
}

extern "C" int tcv_batch_get_relocalization(tcv_batch *b, int window, tcv_relo_result *out) {
    if (!b || !out || window < 0 || window >= b->in.n) { set_error("batch_get_relocalization: bad argument"); return TCV_ERR_INVALID; }
    const ReloState *r = tcv_relo_of(b);
    if (r && !r->have) { set_error("batch_get_relocalization: the states have not been downloaded behind tcv_batch_gauge_fix"); return TCV_ERR_INVALID; }
    if (!r && b->dl.h_state.empty()) { set_error("batch_get_relocalization: the states have not been downloaded"); return TCV_ERR_INVALID; }
    for (int k = 0; r && k < r->n; k++)
        if (r->win[k] == window) { record_to_public(r->h_rec.data() + (size_t)RELO_REC * k, r->valid[k], out); return TCV_OK; }
    record_to_public(nullptr, 0, out);      // a window without relocalisation
    return TCV_OK;
}
