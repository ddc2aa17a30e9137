// Host half of the visual-inertial alignment (include/tcv_vi_alignment.h; the kernels: tcv_align.hip): validation, the two passes through
// the library's pre-integration (tcv_preintegrate: IntegrationBase at (ba0, bg0), then repropagate(0, bg), initial_aligment.cpp:35), the
// two round trips of the alignment's own kernels and the unpacking of the per-sequence records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tcv_vi_alignment.h"
#include "tcv_align.h"
#include "tcv_host.h"
#include "tcv_runtime.h"

using namespace tcv;

namespace {
static_assert(sizeof(AlignHdr) % 8 == 0, "the headers lie in front of doubles");
static_assert(TCV_VI_ALIGN_MAX_FRAMES == 128, "tcv_launch_align_bias sizes its LDS for this many frames");

thread_local double g_al_timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
enum { PRE_CHUNK = 8192 };      // intervals per tcv_preintegrate call: 30 MB of records at a time

bool all_finite(const double *p, size_t n) {
    for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false;
    return true;
}
int bad(int g, const char *what) { set_error("vi_align: sequence " + std::to_string(g) + ": " + what); return TCV_ERR_INVALID; }

int al_validate(const tcv_vi_align_desc &d, const tcv_vi_align_result &r, int g) {
    if (d.n_frames < 2) return bad(g, "n_frames < 2");
    if (!d.R || !d.T || !d.first || !d.count || !d.samples7 || !d.acc0_gyr0 || !d.key_frame) return bad(g, "missing array");
    if (!r.velocity || !r.Ps || !r.Rs || !r.Vs) return bad(g, "missing result array");
    if (d.num_samples < 0) return bad(g, "num_samples < 0");
    if (d.n_frames > TCV_VI_ALIGN_MAX_FRAMES) { set_error("vi_align: sequence " + std::to_string(g) + ": beyond TCV_VI_ALIGN_MAX_FRAMES"); return TCV_ERR_UNSUPPORTED; }
    const int F = d.n_frames;
    if (d.n_key < 1 || d.n_key > F) return bad(g, "n_key out of range");
    for (int k = 0; k < d.n_key; k++) {
        if (d.key_frame[k] < 0 || d.key_frame[k] >= F) return bad(g, "key_frame out of range");
        if (k && d.key_frame[k] <= d.key_frame[k - 1]) return bad(g, "key_frame not strictly ascending");
    }
    for (int i = 0; i < F - 1; i++) {
        if (d.count[i] < 1) return bad(g, "interval without samples");
        if (d.first[i] < 0 || (long long)d.first[i] + d.count[i] > d.num_samples) return bad(g, "sample range out of bounds");
        if (!all_finite(d.samples7 + 7 * (size_t)d.first[i], 7 * (size_t)d.count[i])) return bad(g, "non-finite sample");
    }
    if (!all_finite(d.R, 9 * (size_t)F) || !all_finite(d.T, 3 * (size_t)F) || !all_finite(d.tic, 3) || !all_finite(d.acc0_gyr0, 6 * (size_t)(F - 1)) ||
        !all_finite(d.ba0, 3) || !all_finite(d.bg0, 3) || !all_finite(d.noise, 4))
        return bad(g, "non-finite input");
    return TCV_OK;
}

// One pass of the library's pre-integration over every interval of the batch, at (ba, bg) = (ba0, bg0) of each sequence, or at (0, bg[3 g ..])
// when `bg` is given; `sink(g, i, record)` sees every interval once.  Sequences that share a noise vector go into one call, PRE_CHUNK
// intervals at most (a sequence is never split).
template <class Sink> int preint_pass(int n, const tcv_vi_align_desc *descs, const double *bg, Sink &&sink) {
    std::vector<int> first, count;
    std::vector<double> samples, init;
    std::vector<tcv_imu_preintegration> rec;
    int g0 = 0;
    while (g0 < n) {
        int g1 = g0, n_itv = 0;
        while (g1 < n && std::memcmp(descs[g1].noise, descs[g0].noise, sizeof descs[g0].noise) == 0 && (g1 == g0 || n_itv + descs[g1].n_frames - 1 <= PRE_CHUNK)) {
            n_itv += descs[g1].n_frames - 1;
            g1++;
        }
        first.clear(); count.clear(); samples.clear(); init.clear();
        for (int g = g0; g < g1; g++) {
            const tcv_vi_align_desc &d = descs[g];
            for (int i = 0; i < d.n_frames - 1; i++) {
                first.push_back((int)(samples.size() / 7)); count.push_back(d.count[i]);
                samples.insert(samples.end(), d.samples7 + 7 * (size_t)d.first[i], d.samples7 + 7 * ((size_t)d.first[i] + d.count[i]));
                init.insert(init.end(), d.acc0_gyr0 + 6 * (size_t)i, d.acc0_gyr0 + 6 * (size_t)i + 6);
                for (int k = 0; k < 3; k++) init.push_back(bg ? 0.0 : d.ba0[k]);
                for (int k = 0; k < 3; k++) init.push_back(bg ? bg[3 * (size_t)g + k] : d.bg0[k]);
            }
        }
        if (samples.size() / 7 > (size_t)0x7fffffff) { set_error("vi_align: too many IMU samples in one pre-integration call"); return TCV_ERR_UNSUPPORTED; }
        rec.resize(n_itv);
        if (int rc = tcv_preintegrate(n_itv, first.data(), count.data(), samples.data(), (int)(samples.size() / 7), init.data(), descs[g0].noise, rec.data())) return rc;
        int k = 0;
        for (int g = g0; g < g1; g++)
            for (int i = 0; i < descs[g].n_frames - 1; i++) sink(g, i, rec[k++]);
        g0 = g1;
    }
    return TCV_OK;
}

double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// events around a kernel inside a RoundTrip's launch; ms() after the round trip's wait
struct KernelTimer {
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer() { if (hipEventCreate(&a) != hipSuccess) a = nullptr; if (hipEventCreate(&b) != hipSuccess) b = nullptr; }
    ~KernelTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start(hipStream_t st) { if (a && b) (void)hipEventRecord(a, st); }
    void stop(hipStream_t st) { if (a && b) (void)hipEventRecord(b, st); }
    double ms() const { float v = 0.0f; return (a && b && hipEventElapsedTime(&v, a, b) == hipSuccess) ? v : 0.0; }
};
}  // namespace

extern "C" void tcv_vi_align_options_default(tcv_vi_align_options *o) {
    if (!o) return;
    o->gravity_norm = 9.81007;           // G.z of the reference's configuration (parameters.cpp)
    o->min_relative_pivot = 4e-11;       // the geometric middle of the measured pair (tests/test_vi_alignment_cpu.py)
}

extern "C" int tcv_vi_align_last_timing(double *out) {
    if (!out) { set_error("vi_align_last_timing: bad argument"); return TCV_ERR_INVALID; }
    for (int k = 0; k < 8; k++) out[k] = g_al_timing[k];
    return TCV_OK;
}

extern "C" int tcv_vi_align(int n, const tcv_vi_align_desc *descs, const tcv_vi_align_options *options, tcv_vi_align_result *results, void *hip_stream) {
    if (n < 1 || !descs || !results) { set_error("vi_align: bad argument"); return TCV_ERR_INVALID; }
    tcv_vi_align_options opt;
    tcv_vi_align_options_default(&opt);
    if (options) opt = *options;
    if (!(std::isfinite(opt.gravity_norm) && opt.gravity_norm > 0.0) || !(opt.min_relative_pivot >= 0.0 && opt.min_relative_pivot < 1.0)) {
        set_error("vi_align: options out of range");
        return TCV_ERR_INVALID;
    }
    int worst = TCV_OK;
    for (int g = 0; g < n; g++) {      // every sequence is validated before a limit is reported
        const int rc = al_validate(descs[g], results[g], g);
        if (rc == TCV_ERR_INVALID) return rc;
        if (rc) worst = rc;
    }
    if (worst) return worst;
    if (n > TCV_VI_ALIGN_MAX_BATCH) { set_error("vi_align: beyond TCV_VI_ALIGN_MAX_BATCH"); return TCV_ERR_UNSUPPORTED; }
    if (int rc = device_ready()) return rc;
    for (int k = 0; k < 8; k++) g_al_timing[k] = 0.0;
    auto t0 = std::chrono::steady_clock::now();

    std::vector<AlignHdr> hdrs(n);
    long long n_frames = 0, n_itv = 0, n_keys = 0, n_out = 0;
    int max_F = 2;
    for (int g = 0; g < n; g++) {
        const tcv_vi_align_desc &d = descs[g];
        AlignHdr &H = hdrs[g];
        H.n_frames = d.n_frames; H.n_key = d.n_key; H.o_frame = (int)n_frames; H.o_itv = (int)n_itv; H.o_key = (int)n_keys; H.status_in = 0; H.o_out = n_out;
        std::memcpy(H.tic, d.tic, sizeof H.tic);
        n_frames += d.n_frames; n_itv += d.n_frames - 1; n_keys += d.n_key; n_out += align_out_doubles(d.n_frames, d.n_key);
        max_F = std::max(max_F, d.n_frames);
        tcv_vi_align_result &r = results[g];      // zeros until something is computed
        r.status = 0; r.scale = 0.0; r.min_pivot = 0.0;
        std::memset(r.delta_bg, 0, sizeof r.delta_bg); std::memset(r.bg, 0, sizeof r.bg); std::memset(r.gravity_c0, 0, sizeof r.gravity_c0);
        std::memset(r.gravity, 0, sizeof r.gravity); std::memset(r.rot_diff, 0, sizeof r.rot_diff);
    }
    hipStream_t st = resolve_stream(hip_stream);
    const size_t b_hdr = sizeof(AlignHdr) * (size_t)n, b_R = 72 * (size_t)n_frames, b_T = 24 * (size_t)n_frames;
    g_al_timing[0] += ms_since(t0);

    // ---- pass 1: IntegrationBase at (ba0, bg0); the bias kernel reads jacobian.block<3,3>(O_R, O_BG) and delta_q of every interval
    std::vector<double> bias_in((size_t)AL_BIAS_IN * n_itv);
    t0 = std::chrono::steady_clock::now();
    if (int rc = preint_pass(n, descs, nullptr, [&](int g, int i, const tcv_imu_preintegration &p) {
            double *o = bias_in.data() + (size_t)AL_BIAS_IN * (hdrs[g].o_itv + i);
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) o[3 * r + c] = p.jacobian[(3 + r) * 15 + 12 + c];      // O_R = 3, O_BG = 12
            std::memcpy(o + 9, p.delta_q, 32);
        })) return rc;
    g_al_timing[1] = ms_since(t0);

    // ---- solveGyroscopeBias
    std::vector<double> bg(3 * (size_t)n);
    {
        t0 = std::chrono::steady_clock::now();
        RoundTrip rt(st, b_hdr + b_R + 8 * bias_in.size(), 8 * (size_t)AL_BIAS_OUT * n);
        if (int rc = rt.ready("vi_align (bias)")) return rc;
        char *h = rt.h_in<char>();
        std::memcpy(h, hdrs.data(), b_hdr);
        for (int g = 0; g < n; g++) std::memcpy(h + b_hdr + 72 * (size_t)hdrs[g].o_frame, descs[g].R, 72 * (size_t)descs[g].n_frames);
        std::memcpy(h + b_hdr + b_R, bias_in.data(), 8 * bias_in.size());
        KernelTimer kt;
        int lrc = 0;
        if (int rc = rt.run("vi_align (bias)", [&](hipStream_t s) {
                const char *dv = rt.d_in<char>();
                kt.start(s);
                lrc = tcv_launch_align_bias(n, (const AlignHdr *)dv, (const double *)(dv + b_hdr), (const double *)(dv + b_hdr + b_R), rt.d_out(), opt.min_relative_pivot, (void *)s);
                kt.stop(s);
            })) return rc;
        if (lrc) return hip_fail((hipError_t)lrc, "vi_align (bias kernel launch)");
        g_al_timing[5] = kt.ms();
        const double *o = rt.h_out();
        for (int g = 0; g < n; g++) {
            tcv_vi_align_result &r = results[g];
            const double *og = o + (size_t)AL_BIAS_OUT * g;
            hdrs[g].status_in = (int)og[3];
            r.min_pivot = og[4];
            for (int k = 0; k < 3; k++) {
                if (hdrs[g].status_in == 0) { r.delta_bg[k] = og[k]; r.bg[k] = descs[g].bg0[k] + og[k]; }      // :29-30
                bg[3 * (size_t)g + k] = descs[g].bg0[k] + (hdrs[g].status_in == 0 ? og[k] : 0.0);
            }
        }
        g_al_timing[2] = ms_since(t0);
    }

    // ---- pass 2: repropagate(Vector3d::Zero(), Bgs[0]) (:32-36)
    std::vector<double> pre_in((size_t)AL_PRE_IN * n_itv);
    t0 = std::chrono::steady_clock::now();
    if (int rc = preint_pass(n, descs, bg.data(), [&](int g, int i, const tcv_imu_preintegration &p) {
            double *o = pre_in.data() + (size_t)AL_PRE_IN * (hdrs[g].o_itv + i);
            std::memcpy(o, p.delta_p, 24); std::memcpy(o + 3, p.delta_v, 24); o[6] = p.sum_dt;
            if (results[g].preint) {
                if (hdrs[g].status_in == 0) results[g].preint[i] = p;
                else std::memset(&results[g].preint[i], 0, sizeof p);
            }
        })) return rc;
    g_al_timing[3] = ms_since(t0);

    // ---- LinearAlignment, RefineGravity, the state change
    {
        t0 = std::chrono::steady_clock::now();
        const size_t b_itv = 8 * pre_in.size(), b_key = ((4 * (size_t)n_keys + 7) / 8) * 8;
        RoundTrip rt(st, b_hdr + b_R + b_T + b_itv + b_key, 8 * (size_t)n_out);
        if (int rc = rt.ready("vi_align (alignment)")) return rc;
        char *h = rt.h_in<char>();
        std::memcpy(h, hdrs.data(), b_hdr);
        int *hk = (int *)(h + b_hdr + b_R + b_T + b_itv);
        for (int g = 0; g < n; g++) {
            const tcv_vi_align_desc &d = descs[g];
            std::memcpy(h + b_hdr + 72 * (size_t)hdrs[g].o_frame, d.R, 72 * (size_t)d.n_frames);
            std::memcpy(h + b_hdr + b_R + 24 * (size_t)hdrs[g].o_frame, d.T, 24 * (size_t)d.n_frames);
            std::memcpy(hk + hdrs[g].o_key, d.key_frame, 4 * (size_t)d.n_key);
        }
        std::memcpy(h + b_hdr + b_R + b_T, pre_in.data(), b_itv);
        const size_t lds_bytes = 8 * align_lds_doubles(max_F);
        const AlignOpts ao = {opt.gravity_norm, opt.min_relative_pivot};
        KernelTimer kt;
        int lrc = 0;
        const double t_pack = ms_since(t0);
        if (int rc = rt.run("vi_align (alignment)", [&](hipStream_t s) {
                const char *dv = rt.d_in<char>();
                kt.start(s);
                lrc = tcv_launch_align_solve(n, (const AlignHdr *)dv, (const double *)(dv + b_hdr), (const double *)(dv + b_hdr + b_R), (const double *)(dv + b_hdr + b_R + b_T),
                                             (const int *)(dv + b_hdr + b_R + b_T + b_itv), rt.d_out(), ao, lds_bytes, (void *)s);
                kt.stop(s);
            })) return rc;
        if (lrc) return hip_fail((hipError_t)lrc, "vi_align (alignment kernel launch)");
        g_al_timing[6] = kt.ms();
        g_al_timing[4] = ms_since(t0) - t_pack;
        g_al_timing[0] += t_pack;
        t0 = std::chrono::steady_clock::now();
        const double *o = rt.h_out();
        for (int g = 0; g < n; g++) {
            const tcv_vi_align_desc &d = descs[g];
            tcv_vi_align_result &r = results[g];
            const double *og = o + hdrs[g].o_out;
            const int F = d.n_frames, K = d.n_key;
            r.status = (int)og[0];
            r.scale = og[1];
            std::memcpy(r.gravity_c0, og + 2, 24); std::memcpy(r.gravity, og + 5, 24); std::memcpy(r.rot_diff, og + 8, 72);
            if (hdrs[g].status_in == 0) r.min_pivot = std::min(r.min_pivot, og[17]);
            std::memcpy(r.velocity, og + AL_HEAD, 24 * (size_t)F);
            std::memcpy(r.Ps, og + AL_HEAD + 3 * F, 24 * (size_t)K);
            std::memcpy(r.Rs, og + AL_HEAD + 3 * F + 3 * K, 72 * (size_t)K);
            std::memcpy(r.Vs, og + AL_HEAD + 3 * F + 12 * K, 24 * (size_t)K);
        }
        g_al_timing[0] += ms_since(t0);
    }
    return TCV_OK;
}
