// Batched factor evaluation of include/tcv.h (the parity surface): n independent factors from host arrays, one thread each, in the layout of
// CostFunction::Evaluate (row-major, global block width, 7th column zero).  Each entry point is one round trip on the calling thread's own
// stream (tcv_runtime.h RoundTrip).
#include <hip/hip_runtime.h>

#include <cstring>

#include "tcv_factors.h"
#include "tcv_host.h"

namespace tcv {
__global__ void eval_imu_kernel(int n, const double *consts, const double *params, double G0, double G1, double G2, int use_given,
                                double *sqrt_io, double *res, double *jac, double *work) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double G[3] = {G0, G1, G2};
    const double *pm = params + (size_t)i * 32, *c = consts + (size_t)i * IMU_CONST;
    double *S = sqrt_io + (size_t)i * 225;
    if (!use_given) imu_sqrt_info(c + IMU_COV, S, work + (size_t)i * 450);
    double *w = work + (size_t)i * 450;   // reuse as raw J (15 x 30)
    double rr[15];
    imu_raw(pm, pm + 7, pm + 16, pm + 23, c, G, rr, 1, jac ? w : nullptr, 30);
    for (int r = 0; r < 15; r++) {
        double a = 0;
        for (int s = r; s < 15; s++) a += S[r * 15 + s] * rr[s];
        res[(size_t)i * 15 + r] = a;
    }
    if (!jac) return;
    double *J = jac + (size_t)i * 480;
    const int gofs[4] = {0, 105, 240, 345}, gw[4] = {7, 9, 7, 9}, lc[4] = {0, 6, 15, 21}, lw[4] = {6, 9, 6, 9};
    for (int b = 0; b < 4; b++)
        for (int r = 0; r < 15; r++) {
            for (int cc = 0; cc < lw[b]; cc++) {
                double a = 0;
                for (int s = r; s < 15; s++) a += S[r * 15 + s] * w[s * 30 + lc[b] + cc];
                J[gofs[b] + r * gw[b] + cc] = a;
            }
            if (gw[b] == 7) J[gofs[b] + r * 7 + 6] = 0.0;
        }
}
__global__ void eval_proj_kernel(int n, const double *pts, const double *params, double sqrt_info, double *res, double *jac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *pm = params + (size_t)i * 22;
    double r[2], J[38];
    proj_eval(pm, pm + 7, pm + 14, pm[21], pts + (size_t)i * 6, sqrt_info, r, jac ? J : nullptr, 19);
    res[2 * i] = r[0]; res[2 * i + 1] = r[1];
    if (!jac) return;
    double *o = jac + (size_t)i * 44;   // 2x7 | 2x7 | 2x7 | 2x1
    for (int b = 0; b < 3; b++)
        for (int row = 0; row < 2; row++) {
            for (int c = 0; c < 6; c++) o[b * 14 + row * 7 + c] = J[row * 19 + 6 * b + c];
            o[b * 14 + row * 7 + 6] = 0.0;
        }
    o[42] = J[18]; o[43] = J[19 + 18];
}
__global__ void eval_proj_td_kernel(int n, const double *pts, const double *aux, const double *params, double sqrt_info, double TR, double ROW,
                                    double *res, double *jac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *pm = params + (size_t)i * 23;
    double r[2], J[40];
    proj_td_eval(pm, pm + 7, pm + 14, pm[21], pm[22], pts + (size_t)i * 6, aux + (size_t)i * 8, sqrt_info, TR, ROW, r, jac ? J : nullptr, 20);
    res[2 * i] = r[0]; res[2 * i + 1] = r[1];
    if (!jac) return;
    double *o = jac + (size_t)i * 46;   // 2x7 | 2x7 | 2x7 | 2x1 | 2x1
    for (int b = 0; b < 3; b++)
        for (int row = 0; row < 2; row++) {
            for (int c = 0; c < 6; c++) o[b * 14 + row * 7 + c] = J[row * 20 + 6 * b + c];
            o[b * 14 + row * 7 + 6] = 0.0;
        }
    o[42] = J[18]; o[43] = J[20 + 18]; o[44] = J[19]; o[45] = J[20 + 19];
}
__global__ void eval_line_kernel(int n, const double *line, const double *consts21, const double *params, double *res, double *jac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r[2], J[12];
    line_eval(params + (size_t)i * 7, line + (size_t)i * 9, consts21, consts21 + 9, consts21 + 18, r, jac ? J : nullptr, 6);
    res[2 * i] = r[0]; res[2 * i + 1] = r[1];
    if (!jac) return;
    double *o = jac + (size_t)i * 14;
    for (int row = 0; row < 2; row++) { for (int c = 0; c < 6; c++) o[row * 7 + c] = J[row * 6 + c]; o[row * 7 + 6] = 0.0; }
}
__global__ void pose_plus_kernel(int n, const double *x, const double *d, double *o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pose_plus(x + (size_t)i * 7, d + (size_t)i * 6, o + (size_t)i * 7);
}
}  // namespace tcv
using namespace tcv;

extern "C" int tcv_eval_imu_factors(int n, const tcv_imu_preintegration *pre, const double *params, const double G[3],
                                    int use_given, double *sqrt_io, double *res, double *jac) {
    if (n <= 0 || !pre || !params || !G || !sqrt_io || !res) return TCV_ERR_INVALID;
    if (int rc = device_ready()) return rc;
    // inputs [constants | parameters | sqrt_info], outputs [sqrt_info (the same doubles: in/out) | residuals | Jacobians], and the kernel's
    // 450-double work area per factor, which never leaves the device
    const size_t N = (size_t)n, n_const = N * IMU_CONST, n_par = N * 32, n_sqrt = N * 225, n_res = N * 15, n_jac = jac ? N * 480 : 0;
    RoundTrip rt(util_stream(), 8 * (n_const + n_par + n_sqrt), 8 * (n_sqrt + n_res + n_jac), 8 * N * 450, 8 * n_sqrt);
    if (int rc = rt.ready("eval_imu_factors")) return rc;
    for (int i = 0; i < n; i++) {
        double *D = rt.h_in() + (size_t)i * IMU_CONST;
        const tcv_imu_preintegration &q = pre[i];
        std::memcpy(D, q.delta_p, 24); std::memcpy(D + 3, q.delta_q, 32); std::memcpy(D + 7, q.delta_v, 24);
        std::memcpy(D + 10, q.linearized_ba, 24); std::memcpy(D + 13, q.linearized_bg, 24); D[16] = q.sum_dt;
        const int rc[5][2] = {{0, 9}, {0, 12}, {3, 12}, {6, 9}, {6, 12}};
        int o = 17;
        for (auto &b : rc) for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) D[o++] = q.jacobian[(b[0] + r) * 15 + b[1] + c];
        std::memcpy(D + 62, q.covariance, 225 * 8);
    }
    std::memcpy(rt.h_in() + n_const, params, 8 * n_par);
    std::memcpy(rt.h_out(), sqrt_io, 8 * n_sqrt);
    const double *dc = rt.d_in();
    double *ds = rt.d_out(), *dr = ds + n_sqrt;
    if (int rc = rt.run("eval_imu_factors", [&](hipStream_t st) {
            hipLaunchKernelGGL(eval_imu_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, dc, dc + n_const, G[0], G[1], G[2], use_given, ds, dr,
                               jac ? dr + n_res : nullptr, rt.d_scratch());
        })) return rc;
    std::memcpy(sqrt_io, rt.h_out(), 8 * n_sqrt);
    std::memcpy(res, rt.h_out() + n_sqrt, 8 * n_res);
    if (jac) std::memcpy(jac, rt.h_out() + n_sqrt + n_res, 8 * n_jac);
    return TCV_OK;
}
extern "C" int tcv_eval_projection_factors(int n, const double *pts, const double *params, double sqrt_info, double *res, double *jac) {
    if (n <= 0 || !pts || !params || !res) return TCV_ERR_INVALID;
    if (int rc = device_ready()) return rc;
    const size_t N = (size_t)n, n_jac = jac ? N * 44 : 0;
    RoundTrip rt(util_stream(), 8 * N * (6 + 22), 8 * (N * 2 + n_jac));      // [pts | params] -> [residuals | Jacobians]
    if (int rc = rt.ready("eval_projection_factors")) return rc;
    std::memcpy(rt.h_in(), pts, 8 * N * 6); std::memcpy(rt.h_in() + N * 6, params, 8 * N * 22);
    const double *di = rt.d_in();
    double *dr = rt.d_out();
    if (int rc = rt.run("eval_projection_factors", [&](hipStream_t st) {
            hipLaunchKernelGGL(eval_proj_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, di, di + N * 6, sqrt_info, dr, jac ? dr + N * 2 : nullptr);
        })) return rc;
    std::memcpy(res, rt.h_out(), 8 * N * 2);
    if (jac) std::memcpy(jac, rt.h_out() + N * 2, 8 * n_jac);
    return TCV_OK;
}
extern "C" int tcv_eval_projection_td_factors(int n, const double *pts, const double *aux, const double *params, double sqrt_info,
                                              double TR, double ROW, double *res, double *jac) {
    if (n <= 0 || !pts || !aux || !params || !res || !(ROW > 0)) return TCV_ERR_INVALID;
    if (int rc = device_ready()) return rc;
    const size_t N = (size_t)n, n_jac = jac ? N * 46 : 0;
    RoundTrip rt(util_stream(), 8 * N * (6 + 8 + 23), 8 * (N * 2 + n_jac));      // [pts | aux | params] -> [residuals | Jacobians]
    if (int rc = rt.ready("eval_projection_td_factors")) return rc;
    std::memcpy(rt.h_in(), pts, 8 * N * 6); std::memcpy(rt.h_in() + N * 6, aux, 8 * N * 8); std::memcpy(rt.h_in() + N * 14, params, 8 * N * 23);
    const double *di = rt.d_in();
    double *dr = rt.d_out();
    if (int rc = rt.run("eval_projection_td_factors", [&](hipStream_t st) {
            hipLaunchKernelGGL(eval_proj_td_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, di, di + N * 6, di + N * 14, sqrt_info, TR, ROW, dr,
                               jac ? dr + N * 2 : nullptr);
        })) return rc;
    std::memcpy(res, rt.h_out(), 8 * N * 2);
    if (jac) std::memcpy(jac, rt.h_out() + N * 2, 8 * n_jac);
    return TCV_OK;
}
extern "C" int tcv_eval_line_factors(int n, const double *line, const double K[9], const double R[9], const double T[3],
                                     const double *params, double *res, double *jac) {
    if (n <= 0 || !line || !K || !R || !T || !params || !res) return TCV_ERR_INVALID;
    if (int rc = device_ready()) return rc;
    const size_t N = (size_t)n, n_jac = jac ? N * 14 : 0;
    RoundTrip rt(util_stream(), 8 * (21 + N * (9 + 7)), 8 * (N * 2 + n_jac));      // [K 9 | R 9 | T 3 | lines | params] -> [residuals | Jacobians]
    if (int rc = rt.ready("eval_line_factors")) return rc;
    double *h = rt.h_in();
    std::memcpy(h, K, 72); std::memcpy(h + 9, R, 72); std::memcpy(h + 18, T, 24);
    std::memcpy(h + 21, line, 8 * N * 9); std::memcpy(h + 21 + N * 9, params, 8 * N * 7);
    const double *di = rt.d_in();
    double *dr = rt.d_out();
    if (int rc = rt.run("eval_line_factors", [&](hipStream_t st) {
            hipLaunchKernelGGL(eval_line_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, di + 21, di, di + 21 + N * 9, dr, jac ? dr + N * 2 : nullptr);
        })) return rc;
    std::memcpy(res, rt.h_out(), 8 * N * 2);
    if (jac) std::memcpy(jac, rt.h_out() + N * 2, 8 * n_jac);
    return TCV_OK;
}
extern "C" int tcv_pose_plus(int n, const double *x, const double *delta, double *out) {
    if (n <= 0 || !x || !delta || !out) return TCV_ERR_INVALID;
    if (int rc = device_ready()) return rc;
    const size_t N = (size_t)n;
    RoundTrip rt(util_stream(), 8 * N * (7 + 6), 8 * N * 7);      // [x | delta] -> [x (+) delta]
    if (int rc = rt.ready("pose_plus")) return rc;
    std::memcpy(rt.h_in(), x, 8 * N * 7); std::memcpy(rt.h_in() + N * 7, delta, 8 * N * 6);
    const double *di = rt.d_in();
    double *dout = rt.d_out();
    if (int rc = rt.run("pose_plus", [&](hipStream_t st) {
            hipLaunchKernelGGL(pose_plus_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, di, di + N * 7, dout);
        })) return rc;
    std::memcpy(out, rt.h_out(), 8 * N * 7);
    return TCV_OK;
}
