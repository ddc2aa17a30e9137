// Host half of the batched bundle adjustment (include/tcv_sfm_ba.h; the kernels: tcv_sfm_ba.hip): validation, the plan of every problem
// (observations in point order, the per-frame lists, the camera columns), one upload, one launch, one download, the world-frame pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tcv_sfm_ba.h"
#include "tcv_runtime.h"
#include "tcv_sfm_ba.h"

using namespace tcv;

namespace {
static_assert(sizeof(BaHdr) % 8 == 0, "the headers lie in front of doubles");
static_assert(BA_T == TCV_SFM_BA_MAX_TRACE, "the summary record holds the public trace");
static_assert(6 * TCV_SFM_BA_MAX_FRAMES - 6 == BA_MAX_NC, "the tile owners cover the largest reduced camera system");
const long long BA_MAX_SCRATCH_BYTES = 2LL << 30;

thread_local double g_ba_timing[4] = {0, 0, 0, 0};      // host packing, upload, kernel, download of the calling thread's last batch, ms

bool all_finite(const double *p, size_t n) {
    for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false;
    return true;
}
int bad(int g, const char *what) { set_error("sfm_ba: problem " + std::to_string(g) + ": " + what); return TCV_ERR_INVALID; }

int ba_validate(const tcv_sfm_ba_desc &d, int g) {
    if (d.n_frames < 2) return bad(g, "n_frames < 2");
    if (d.l < 0 || d.l >= d.n_frames) return bad(g, "l out of range");
    if (d.n_points < 1) return bad(g, "n_points < 1");
    if (d.n_obs < 0) return bad(g, "n_obs < 0");
    if (!d.c_rotation || !d.c_translation || !d.position || !d.obs_first || !d.obs_count || !d.obs_frame || !d.obs_uv) return bad(g, "missing array");
    const bool many_frames = d.n_frames > TCV_SFM_BA_MAX_FRAMES;
    for (int p = 0; p < d.n_points; p++) {
        const int o0 = d.obs_first[p], cnt = d.obs_count[p];
        if (cnt < 2) return bad(g, "a point with fewer than 2 observations");
        if (o0 < 0 || (long long)o0 + cnt > d.n_obs) return bad(g, "observation range out of bounds");
        unsigned long long seen[4] = {0, 0, 0, 0};
        for (int o = o0; o < o0 + cnt; o++) {
            const int f = d.obs_frame[o];
            if (f < 0 || f >= d.n_frames) return bad(g, "frame index out of range");
            if (many_frames) continue;      // (reported as a limit below; the duplicate test needs the frame to fit the mask)
            if (seen[f >> 6] >> (f & 63) & 1) return bad(g, "a point sees the same frame twice");
            seen[f >> 6] |= 1ull << (f & 63);
        }
        if (!all_finite(d.obs_uv + 2 * (size_t)o0, 2 * (size_t)cnt)) return bad(g, "non-finite input");
    }
    if (!all_finite(d.c_rotation, 4 * (size_t)d.n_frames) || !all_finite(d.c_translation, 3 * (size_t)d.n_frames) || !all_finite(d.position, 3 * (size_t)d.n_points))
        return bad(g, "non-finite input");
    for (int i = 0; i < d.n_frames; i++) {
        const double *q = d.c_rotation + 4 * i;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return bad(g, "zero quaternion");
    }
    if (many_frames || d.n_points > TCV_SFM_BA_MAX_POINTS) {
        set_error("sfm_ba: problem " + std::to_string(g) + ": beyond TCV_SFM_BA_MAX_FRAMES / TCV_SFM_BA_MAX_POINTS");
        return TCV_ERR_UNSUPPORTED;
    }
    return TCV_OK;
}
int ba_validate_result(const tcv_sfm_ba_result &r, int g) { return (!r.c_rotation || !r.c_translation || !r.position) ? bad(g, "missing result array") : (int)TCV_OK; }

struct BaPlan {
    int F = 0, P = 0, NO = 0, nc = 0;
    std::vector<int> ints;      // tcv_sfm_ba.h: obs_frame | obs_point | point_first | frame_ptr | frame_obs | coff | colinfo
    std::vector<int> src;       // the caller's observation behind every packed one
};
void ba_plan(const tcv_sfm_ba_desc &d, BaPlan &P) {
    const int F = d.n_frames, N = d.n_points;
    std::vector<int> ofr, opt, pfirst(N + 1, 0), coff(2 * F, -1), colinfo;
    P.src.clear();
    for (int p = 0; p < N; p++) {
        pfirst[p] = (int)ofr.size();
        for (int o = d.obs_first[p]; o < d.obs_first[p] + d.obs_count[p]; o++) { ofr.push_back(d.obs_frame[o]); opt.push_back(p); P.src.push_back(o); }
    }
    const int NO = pfirst[N] = (int)ofr.size();
    std::vector<int> fptr(F + 1, 0), fobs(NO);
    for (int o = 0; o < NO; o++) fptr[ofr[o] + 1]++;
    for (int f = 0; f < F; f++) fptr[f + 1] += fptr[f];
    {
        std::vector<int> at(fptr.begin(), fptr.end() - 1);
        for (int o = 0; o < NO; o++) fobs[at[ofr[o]]++] = o;
    }
    // :248-255: c_rotation[l], c_translation[l] and c_translation[F - 1] are constant
    for (int f = 0; f < F; f++) {
        if (f != d.l) { coff[2 * f] = (int)colinfo.size(); for (int k = 0; k < 3; k++) colinfo.push_back(6 * f + k); }
        if (f != d.l && f != F - 1) { coff[2 * f + 1] = (int)colinfo.size(); for (int k = 3; k < 6; k++) colinfo.push_back(6 * f + k); }
    }
    P.F = F; P.P = N; P.NO = NO; P.nc = (int)colinfo.size();
    P.ints.clear();
    for (const std::vector<int> *v : {&ofr, &opt, &pfirst, &fptr, &fobs, &coff, &colinfo}) P.ints.insert(P.ints.end(), v->begin(), v->end());
}

BaOpts ba_opts(const tcv_sfm_ba_options &d) {
    BaOpts r;
    r.max_it = d.max_num_iterations; r.max_invalid = d.max_num_consecutive_invalid_steps;
    r.ftol = d.function_tolerance; r.gtol = d.gradient_tolerance; r.ptol = d.parameter_tolerance; r.radius0 = d.initial_trust_region_radius;
    r.min_rel_dec = d.min_relative_decrease;
    return r;
}
int ba_check_opts(const tcv_sfm_ba_options &o) {
    const double v[] = {o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius, o.min_relative_decrease, o.accept_cost};
    for (double x : v) if (!std::isfinite(x)) { set_error("sfm_ba: non-finite option"); return TCV_ERR_INVALID; }
    if (o.max_num_iterations < 0 || o.max_num_consecutive_invalid_steps < 1 || !(o.initial_trust_region_radius > 0.0)) { set_error("sfm_ba: bad option"); return TCV_ERR_INVALID; }
    return TCV_OK;
}

// :290-303 on the host, in the order the header states; no contraction, so that the pair is a function of the three arrays alone
#pragma clang fp contract(off)
void ba_world_frame(int F, const double *c_rotation, const double *c_translation, double *q, double *T) {
    for (int i = 0; i < F; i++) {
        const double *r = c_rotation + 4 * i, *c = c_translation + 3 * i;
        const double n = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3];
        const double w = r[0] / n, x = -r[1] / n, y = -r[2] / n, z = -r[3] / n;
        if (q) { q[4 * i] = w; q[4 * i + 1] = x; q[4 * i + 2] = y; q[4 * i + 3] = z; }
        if (T) {
            const double u0 = 2.0 * (y * c[2] - z * c[1]), u1 = 2.0 * (z * c[0] - x * c[2]), u2 = 2.0 * (x * c[1] - y * c[0]);
            T[3 * i] = -((c[0] + w * u0) + (y * u2 - z * u1));
            T[3 * i + 1] = -((c[1] + w * u1) + (z * u0 - x * u2));
            T[3 * i + 2] = -((c[2] + w * u2) + (x * u1 - y * u0));
        }
    }
}
}  // namespace

extern "C" void tcv_sfm_ba_options_default(tcv_sfm_ba_options *o) {
    if (!o) return;
    o->max_num_iterations = 50; o->max_num_consecutive_invalid_steps = 5;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4; o->min_relative_decrease = 1e-3; o->accept_cost = 5e-3;
}

extern "C" int tcv_sfm_ba_plan_stats(const tcv_sfm_ba_desc *desc, long long *out) {
    if (!desc || !out) { set_error("sfm_ba_plan_stats: bad argument"); return TCV_ERR_INVALID; }
    if (int rc = ba_validate(*desc, 0)) return rc;
    BaPlan P;
    ba_plan(*desc, P);
    out[0] = P.nc; out[1] = P.P; out[2] = P.NO; out[3] = 8 * (long long)ba_lds_doubles(P.nc, P.F); out[4] = 8 * ba_scratch_doubles(P.F, P.P, P.NO, P.nc);
    out[5] = ba_ncp(P.nc); out[6] = BA_CHUNK; out[7] = 0;
    return TCV_OK;
}

extern "C" int tcv_sfm_ba_last_timing(double *out) {
    if (!out) { set_error("sfm_ba_last_timing: bad argument"); return TCV_ERR_INVALID; }
    for (int k = 0; k < 4; k++) out[k] = g_ba_timing[k];
    return TCV_OK;
}

extern "C" int tcv_sfm_ba(int n, const tcv_sfm_ba_desc *descs, const tcv_sfm_ba_options *options, tcv_sfm_ba_result *results, void *hip_stream) {
    if (n < 1 || !descs || !results) { set_error("sfm_ba: bad argument"); return TCV_ERR_INVALID; }
    tcv_sfm_ba_options opt;
    tcv_sfm_ba_options_default(&opt);
    if (options) opt = *options;
    if (int rc = ba_check_opts(opt)) return rc;
    int worst = TCV_OK;
    for (int g = 0; g < n; g++) {      // every problem is validated before a limit is reported
        int rc = ba_validate(descs[g], g);
        if (rc != TCV_ERR_INVALID) if (int r2 = ba_validate_result(results[g], g)) rc = r2;
        if (rc == TCV_ERR_INVALID) return rc;
        if (rc) worst = rc;
    }
    if (worst) return worst;
    if (n > TCV_SFM_BA_MAX_BATCH) { set_error("sfm_ba: beyond TCV_SFM_BA_MAX_BATCH"); return TCV_ERR_UNSUPPORTED; }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<BaPlan> plans(n);
    std::vector<BaHdr> hdrs(n);
    long long n_int = 0, n_dbl = 0, n_scr = 0, n_out = 0;
    int max_nc = 0, max_F = 2;
    for (int g = 0; g < n; g++) {
        ba_plan(descs[g], plans[g]);
        const BaPlan &P = plans[g];
        BaHdr &H = hdrs[g];
        H.n_frames = P.F; H.n_points = P.P; H.n_obs = P.NO; H.nc = P.nc;
        H.o_int = n_int; H.o_dbl = n_dbl; H.o_scr = n_scr; H.o_out = n_out;
        n_int += (long long)P.ints.size();
        n_dbl += ba_nx(P.F, P.P) + 2LL * P.NO;
        n_scr += ba_scratch_doubles(P.F, P.P, P.NO, P.nc);
        n_out += ba_nx(P.F, P.P) + BA_SUM;
        max_nc = std::max(max_nc, P.nc); max_F = std::max(max_F, P.F);
    }
    if (8 * n_scr > BA_MAX_SCRATCH_BYTES) { set_error("sfm_ba: the batch needs more than 2 GiB of device scratch"); return TCV_ERR_UNSUPPORTED; }
    if (int rc = device_ready()) return rc;
    // one upload: [headers | input doubles | ints], one device allocation: [upload | output | scratch]
    const size_t b_hdr = sizeof(BaHdr) * (size_t)n, b_dbl = 8 * (size_t)n_dbl, b_int = ((4 * (size_t)n_int + 7) / 8) * 8;
    const size_t b_in = b_hdr + b_dbl + b_int, b_out = 8 * (size_t)n_out, b_scr = 8 * (size_t)n_scr;
    hipStream_t st = resolve_stream(hip_stream);
    StagedTransfer tr(st, b_in + b_out);
    if (!tr.host) { set_error("hipHostMalloc (sfm_ba staging) failed"); return TCV_ERR_HIP; }
    char *h = (char *)tr.host;
    std::memcpy(h, hdrs.data(), b_hdr);
    double *hd = (double *)(h + b_hdr);
    int *hi = (int *)(h + b_hdr + b_dbl);
    for (int g = 0; g < n; g++) {
        const tcv_sfm_ba_desc &d = descs[g];
        const BaPlan &P = plans[g];
        double *p = hd + hdrs[g].o_dbl;
        std::memcpy(p, d.c_rotation, 32 * (size_t)P.F); p += 4 * P.F;
        std::memcpy(p, d.c_translation, 24 * (size_t)P.F); p += 3 * P.F;
        std::memcpy(p, d.position, 24 * (size_t)P.P); p += 3 * P.P;
        for (int o = 0; o < P.NO; o++) { p[2 * o] = d.obs_uv[2 * (size_t)P.src[o]]; p[2 * o + 1] = d.obs_uv[2 * (size_t)P.src[o] + 1]; }
        std::memcpy(hi + hdrs[g].o_int, P.ints.data(), sizeof(int) * P.ints.size());
    }
    const auto t1 = std::chrono::steady_clock::now();
    hipError_t e = tr.dev_alloc(b_in + b_out + b_scr);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (sfm_ba batch)");
    char *dv = (char *)tr.dev;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = true;
    for (int k = 0; k < 4; k++) timed = timed && hipEventCreate(&ev[k]) == hipSuccess;
    tr.issued();
    if (timed) (void)hipEventRecord(ev[0], st);
    e = hipMemcpyAsync(dv, h, b_in, hipMemcpyHostToDevice, st);
    if (timed) (void)hipEventRecord(ev[1], st);
    if (e == hipSuccess)
        e = (hipError_t)tcv_launch_sfm_ba(n, (const BaHdr *)dv, (const int *)(dv + b_hdr + b_dbl), (const double *)(dv + b_hdr), (double *)(dv + b_in + b_out),
                                          (double *)(dv + b_in), ba_opts(opt), 8 * ba_lds_doubles(max_nc, max_F), (void *)st);
    if (timed) (void)hipEventRecord(ev[2], st);
    if (e == hipSuccess) e = hipMemcpyAsync(h + b_in, dv + b_in, b_out, hipMemcpyDeviceToHost, st);
    if (timed) (void)hipEventRecord(ev[3], st);
    if (e == hipSuccess) e = tr.wait();
    g_ba_timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    for (int k = 0; k < 3; k++) {
        float ms = 0.0f;
        if (timed && e == hipSuccess && hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_ba_timing[1 + k] = ms; else g_ba_timing[1 + k] = 0.0;
    }
    for (int k = 0; k < 4; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (e != hipSuccess) return hip_fail(e, "sfm_ba");
    const double *ho = (const double *)(h + b_in);
    for (int g = 0; g < n; g++) {
        const BaPlan &P = plans[g];
        const double *o = ho + hdrs[g].o_out, *s = o + ba_nx(P.F, P.P);
        tcv_sfm_ba_result &r = results[g];
        std::memcpy(r.c_rotation, o, 32 * (size_t)P.F);
        std::memcpy(r.c_translation, o + 4 * P.F, 24 * (size_t)P.F);
        std::memcpy(r.position, o + 7 * P.F, 24 * (size_t)P.P);
        if (r.q || r.T) ba_world_frame(P.F, r.c_rotation, r.c_translation, r.q, r.T);
        tcv_sfm_ba_summary &S = r.summary;
        std::memset(&S, 0, sizeof S);
        S.iterations = (int)s[2]; S.termination = (int)s[3];
        S.num_camera_unknowns = P.nc; S.num_points = P.P; S.num_observations = P.NO;
        S.initial_cost = s[0]; S.final_cost = s[1];
        S.accepted = ((S.termination >= 1 && S.termination <= 4) || S.final_cost < opt.accept_cost) ? 1 : 0;      // :281
        for (int k = 0; k < BA_T; k++) {
            S.cost[k] = s[4 + k]; S.cost_candidate[k] = s[4 + BA_T + k]; S.rho[k] = s[4 + 2 * BA_T + k]; S.radius[k] = s[4 + 3 * BA_T + k];
            S.step[k] = (int)s[4 + 4 * BA_T + k];
        }
    }
    return TCV_OK;
}

extern "C" int tcv_sfm_ba_eval_observations(int n, const double *rotation, const double *translation, const double *point, const double *uv,
                                            double *residual, double *jacobian, double *cost) {
    if (n < 1 || n > (1 << 20) || !rotation || !translation || !point || !uv || !residual || !jacobian || !cost) { set_error("sfm_ba_eval_observations: bad argument"); return TCV_ERR_INVALID; }
    std::vector<double> in((size_t)BA_OBS_IN * n);
    for (int i = 0; i < n; i++) {
        double *c = in.data() + (size_t)BA_OBS_IN * i;
        std::memcpy(c, rotation + 4 * (size_t)i, 32); std::memcpy(c + 4, translation + 3 * (size_t)i, 24); std::memcpy(c + 7, point + 3 * (size_t)i, 24);
        std::memcpy(c + 10, uv + 2 * (size_t)i, 16);
        if (!(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3] > 0.0)) { set_error("sfm_ba_eval_observations: zero or non-finite quaternion"); return TCV_ERR_INVALID; }
    }
    if (!all_finite(in.data(), in.size())) { set_error("sfm_ba_eval_observations: non-finite input"); return TCV_ERR_INVALID; }
    if (int rc = device_ready()) return rc;
    RoundTrip rt(util_stream(), 8 * in.size(), 8 * (size_t)BA_OBS_OUT * n);
    if (int rc = rt.ready("sfm_ba_eval_observations")) return rc;
    std::memcpy(rt.h_in<char>(), in.data(), 8 * in.size());
    int lrc = 0;
    if (int rc = rt.run("sfm_ba_eval_observations", [&](hipStream_t s) { lrc = tcv_launch_sfm_ba_observations(n, rt.d_in(), rt.d_out(), (void *)s); })) return rc;
    if (lrc) return hip_fail((hipError_t)lrc, "sfm_ba_eval_observations (launch)");
    const double *o = rt.h_out();
    for (int i = 0; i < n; i++) {
        std::memcpy(residual + 2 * (size_t)i, o + (size_t)BA_OBS_OUT * i, 16);
        std::memcpy(jacobian + 18 * (size_t)i, o + (size_t)BA_OBS_OUT * i + 2, 144);
        cost[i] = o[(size_t)BA_OBS_OUT * i + 20];
    }
    return TCV_OK;
}
