// Visual-inertial alignment (include/tcv_vi_alignment.h): VisualIMUAlignment of the reference (vins_estimator/src/initial/initial_aligment.cpp)
// and the state change of Estimator::visualInitialAlign (estimator.cpp:1380-1438), one single-wavefront workgroup per sequence.
//
//   align_bias_kernel    solveGyroscopeBias (:3-27) up to delta_bg; the re-propagation (:32-36) is the pre-integration kernel's second launch
//   align_solve_kernel   LinearAlignment (:125-197), RefineGravity (:55-123), TangentBasis (:40-53), the state change, g2R (utility.cpp:3-13)
//
// The normal matrix of LinearAlignment is block-tridiagonal in the velocities (scalar half-bandwidth 5) with a dense border of 4 rows
// [g | 100 s]; RefineGravity's has the same velocity block and the border [dg 2 | 100 s].  So the band is assembled and factored ONCE, in
// place in LDS; each of the five solves (LinearAlignment + four rounds) rebuilds only the border rows that depend on lxly / g0 and the
// right-hand side, pushes them through the factor, forms and factors the border's Schur complement and substitutes back: a natural-order
// Cholesky of the whole matrix, entry by entry.  Every sum has one order (intervals ascending, inside an interval the six rows of tmp_A
// ascending; eliminations ascending), nothing is atomic and a workgroup reads nothing of its neighbours: a sequence's bits do not depend
// on the batch.
#include <hip/hip_runtime.h>

#include "tcv_align.h"
#include "tcv_dev.h"
#include "tcv_gauge.h"

namespace tcv {

// tmp_A(k, p) of an interval's record for the velocity columns p < 6 (:149-156): rows 0..2 [-dt I | 0], rows 3..5 [-I | Ri' Rj]
__device__ __forceinline__ double al_a(const lds_d *r, int k, int p) {
    if (k < 3) return (p == k) ? -r[0] : 0.0;
    if (p < 3) return (p == k - 3) ? -1.0 : 0.0;
    return r[1 + 3 * (k - 3) + (p - 3)];
}
// border column a < AL_NB of tmp_A, or tmp_b (a == AL_NB)
__device__ __forceinline__ double al_x(const lds_d *r, int k, int a) { return a < AL_NB ? r[10 + AL_NB * k + a] : r[34 + k]; }
// r_A(p, q) = sum_k tmp_A(k, p) tmp_A(k, q) (:165-166; cov_inv = I), k ascending
__device__ __forceinline__ double al_rvv(const lds_d *r, int p, int q) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += al_a(r, k, p) * al_a(r, k, q);
    return s;
}
__device__ __forceinline__ double al_rvx(const lds_d *r, int p, int a) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += al_a(r, k, p) * al_x(r, k, a);
    return s;
}
__device__ __forceinline__ double al_rxx(const lds_d *r, int a, int b) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += al_x(r, k, a) * al_x(r, k, b);
    return s;
}
__device__ __forceinline__ V3 al_normalized(V3 v) {      // Eigen's normalized(): v / sqrt(squaredNorm) when the latter is positive
    const double z = dot(v, v);
    return z > 0.0 ? v / sqrt(z) : v;
}
__device__ __forceinline__ bool al_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-Inf
// Utility::g2R (utility.cpp:3-13).  Quaterniond::FromTwoVectors(ng1, z): axis = v0 x v1, w from sqrt(2 (1 + c)) as Eigen does; in the
// antiparallel branch (c < -1 + 1e-12) Eigen takes the axis from an SVD of [v0; v1] -- here the fixed unit axis (1, 0, 0), perpendicular to z.
__device__ __forceinline__ M3 al_g2R(V3 g) {
    const V3 ng1 = al_normalized(g), v0 = al_normalized(ng1), v1(0.0, 0.0, 1.0);
    const double c = dot(v1, v0);
    Quat q;
    if (c < -1.0 + 1e-12) {
        const double w2 = fmax((1.0 + c) * 0.5, 0.0), sv = sqrt(1.0 - w2);
        q = Quat(sv, 0.0, 0.0, sqrt(w2));
    } else {
        const V3 axis = cross(v0, v1);
        const double s = sqrt((1.0 + c) * 2.0), invs = 1.0 / s;
        q = Quat(axis.x * invs, axis.y * invs, axis.z * invs, s * 0.5);
    }
    const M3 R0 = to_matrix(q);
    double ypr[3];
    r2ypr(R0, ypr);
    return ypr2R(-ypr[0], 0.0, 0.0) * R0;
}

// misc (64 doubles at the end of LDS): the border system S(a, b) at 5 a + b, b == 4 the right-hand side | xb 4 | g0 3 | lx 3 | ly 3 | fail flag |
// smallest relative pivot | the border's diagonal before elimination 4
enum { MI_S = 0, MI_XB = 20, MI_G0 = 24, MI_LX = 27, MI_LY = 30, MI_FAIL = 33, MI_PIV = 34, MI_C0 = 36 };

__global__ void __launch_bounds__(AL_THREADS) align_solve_kernel(int n_seq, const AlignHdr *hdrs, const double *Rg, const double *Tg, const double *itv,
                                                                 const int *keys, double *out, AlignOpts opt) {
    extern __shared__ __attribute__((aligned(16))) double al_lds_raw[];
    const int tid = threadIdx.x, seq = blockIdx.x;
    if (seq >= n_seq) return;
    const AlignHdr H = hdrs[seq];
    const int F = H.n_frames, K = H.n_key, n = 3 * F, NV = n + AL_NB, NI = F - 1;
    lds_d *band = (lds_d *)al_lds_raw, *diag0 = band + n * AL_BANDW, *vec = diag0 + n, *rec = vec + AL_NVEC * NV, *misc = rec + AL_REC * NI;
    lds_d *xv = vec + AL_NB * NV;      // the right-hand side, then the solution's velocities
    const double *R = Rg + 9 * (size_t)H.o_frame, *T = Tg + 3 * (size_t)H.o_frame, *P = itv + (size_t)AL_PRE_IN * H.o_itv;
    const int *key = keys + H.o_key;
    double *O = out + H.o_out;
    const int n_out = AL_HEAD + 3 * F + 15 * K;      // align_out_doubles
    const V3 tic(H.tic[0], H.tic[1], H.tic[2]);
    const double G = opt.gravity_norm;
    if (H.status_in != 0) {      // the gyroscope bias was not found: nothing after it is computed
        for (int i = tid; i < n_out; i += AL_THREADS) O[i] = (i == 0) ? (double)H.status_in : 0.0;
        return;
    }
    if (tid == 0) { misc[MI_FAIL] = 0.0; misc[MI_PIV] = 1.0; }
    if (tid < 9) misc[MI_G0 + tid] = 0.0;
    __syncthreads();

    // the per-interval records.  refine == false: LinearAlignment's tmp_A (6 x 10) and tmp_b (:149-157); true: RefineGravity's (6 x 9, :87-95) with
    // the scale column kept at border index 3 and border index 2 empty
    auto build_records = [&](bool refine) {
        const V3 g0(misc[MI_G0], misc[MI_G0 + 1], misc[MI_G0 + 2]), lx(misc[MI_LX], misc[MI_LX + 1], misc[MI_LX + 2]), ly(misc[MI_LY], misc[MI_LY + 1], misc[MI_LY + 2]);
        for (int i = tid; i < NI; i += AL_THREADS) {
            const M3 Rit = transpose(m3_load(R + 9 * i)), Rj = m3_load(R + 9 * (i + 1));
            const M3 RtR = Rit * Rj;
            const double dt = P[AL_PRE_IN * i + 6];
            const V3 dp(P + AL_PRE_IN * i), dv(P + AL_PRE_IN * i + 3);
            M3 G1, G2;      // Ri' * dt * dt / 2 and Ri' * dt, evaluated left to right as Eigen does
#pragma unroll
            for (int e = 0; e < 9; e++) { G1.m[e] = Rit.m[e] * dt * dt / 2; G2.m[e] = Rit.m[e] * dt; }
            const V3 c9 = (Rit * (V3(T + 3 * (i + 1)) - V3(T + 3 * i))) / 100.0;
            V3 bp = dp + RtR * tic - tic, bv = dv;
            lds_d *r = rec + AL_REC * i;
            r[0] = dt;
#pragma unroll
            for (int e = 0; e < 9; e++) r[1 + e] = RtR.m[e];
            if (!refine) {
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int a = 0; a < 3; a++) { r[10 + AL_NB * k + a] = G1.m[3 * k + a]; r[10 + AL_NB * (3 + k) + a] = G2.m[3 * k + a]; }
            } else {
                const V3 p0 = G1 * lx, p1 = G1 * ly, v0 = G2 * lx, v1 = G2 * ly;      // tmp_A.block<3,2>(0, 6) and (3, 6)
                bp = bp - G1 * g0;
                bv = dv - G2 * g0;
                r[10] = p0.x; r[14] = p0.y; r[18] = p0.z; r[11] = p1.x; r[15] = p1.y; r[19] = p1.z; r[12] = r[16] = r[20] = 0.0;
                r[22] = v0.x; r[26] = v0.y; r[30] = v0.z; r[23] = v1.x; r[27] = v1.y; r[31] = v1.z; r[24] = r[28] = r[32] = 0.0;
            }
            r[13] = c9.x; r[17] = c9.y; r[21] = c9.z; r[25] = r[29] = r[33] = 0.0;
            r[34] = bp.x; r[35] = bp.y; r[36] = bp.z; r[37] = bv.x; r[38] = bv.y; r[39] = bv.z;
        }
        __syncthreads();
    };

    // the border rows in `mask` (bit a; bit AL_NB: the right-hand side) over the velocity columns, and the border-border block with its
    // right-hand side (:168-175), all x 1000 (:177-178)
    auto assemble_vectors = [&](unsigned mask) {
        for (int a = 0; a < AL_NVEC; a++) {
            if (!(mask >> a & 1)) continue;
            for (int c = tid; c < n; c += AL_THREADS) {
                const int f = c / 3, e = c - 3 * f;
                double v = 0.0;
                if (f >= 1) v += al_rvx(rec + AL_REC * (f - 1), 3 + e, a);
                if (f <= F - 2) v += al_rvx(rec + AL_REC * f, e, a);
                vec[a * NV + c] = v * 1000.0;
            }
        }
        if (tid < AL_NB * AL_NVEC) {
            const int a = tid / AL_NVEC, b = tid - AL_NVEC * a;
            double v = 0.0;
            for (int i = 0; i < NI; i++) v += al_rxx(rec + AL_REC * i, a, b);
            misc[MI_S + tid] = v * 1000.0;
            if (a == b) misc[MI_C0 + a] = v * 1000.0;
        }
        __syncthreads();
    };

    // L y = v for the vectors in `mask`, in place, column by column: lane a divides, lanes (a, q) eliminate
    auto forward = [&](unsigned mask) {
        const int a = tid / AL_BW, q = tid - AL_BW * a + 1;
        const bool mine = tid < AL_NVEC * AL_BW && (mask >> a & 1), head = tid < AL_NVEC && (mask >> tid & 1);
        for (int j = 0; j < n; j++) {
            if (head) vec[tid * NV + j] = vec[tid * NV + j] / band[j * AL_BANDW + AL_BW];
            __syncthreads();
            if (mine && j + q < n) vec[a * NV + j + q] -= band[(j + q) * AL_BANDW + AL_BW - q] * vec[a * NV + j];
            __syncthreads();
        }
    };

    // Schur complement of the border (nb == 4: indices 0 1 2 3, nb == 3: 0 1 3), its Cholesky behind the rank gate, the border's solution into
    // misc[MI_XB ..], then the velocities into xv.  A failed gate raises misc[MI_FAIL].
    auto solve_border_and_back = [&](int nb) {
        if (tid < AL_NB * AL_NVEC) {
            const int a = tid / AL_NVEC, b = tid - AL_NVEC * a;
            double s = misc[MI_S + tid];
            const lds_d *ya = vec + a * NV, *yb = vec + b * NV;
            for (int j = 0; j < n; j++) s -= ya[j] * yb[j];
            misc[MI_S + tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            auto o = [&](int i) { return (nb == AL_NB || i < 2) ? i : 3; };
            bool fail = false;
            double piv = misc[MI_PIV];
            for (int i = 0; i < nb && !fail; i++) {
                const int oi = o(i);
                const double d = misc[MI_S + AL_NVEC * oi + oi], a0 = misc[MI_C0 + oi];
                if (!(d > opt.min_relative_pivot * a0)) { fail = true; break; }
                piv = fmin(piv, d / a0);
                const double l = sqrt(d);
                misc[MI_S + AL_NVEC * oi + oi] = l;
                misc[MI_S + AL_NVEC * oi + AL_NB] = misc[MI_S + AL_NVEC * oi + AL_NB] / l;
                for (int r = i + 1; r < nb; r++) misc[MI_S + AL_NVEC * o(r) + oi] = misc[MI_S + AL_NVEC * o(r) + oi] / l;
                for (int r = i + 1; r < nb; r++) {
                    const int orr = o(r);
                    const double lr = misc[MI_S + AL_NVEC * orr + oi];
                    for (int c = i + 1; c <= r; c++) misc[MI_S + AL_NVEC * orr + o(c)] -= lr * misc[MI_S + AL_NVEC * o(c) + oi];
                    misc[MI_S + AL_NVEC * orr + AL_NB] -= lr * misc[MI_S + AL_NVEC * oi + AL_NB];
                }
            }
            for (int i = 0; i < AL_NB; i++) misc[MI_XB + i] = 0.0;
            for (int i = nb - 1; i >= 0 && !fail; i--) {
                const int oi = o(i);
                double x = misc[MI_S + AL_NVEC * oi + AL_NB];
                for (int r = i + 1; r < nb; r++) x -= misc[MI_S + AL_NVEC * o(r) + oi] * misc[MI_XB + o(r)];
                misc[MI_XB + oi] = x / misc[MI_S + AL_NVEC * oi + oi];
            }
            misc[MI_PIV] = piv;
            if (fail) misc[MI_FAIL] = 1.0;
        }
        __syncthreads();
        if (misc[MI_FAIL] != 0.0) return;
        // z - sum_a y_a xb_a, border index ascending; then L' x = that, column by column from the last
        for (int j = tid; j < n; j += AL_THREADS) {
            double t = xv[j];
            for (int i = 0; i < nb; i++) { const int a = (nb == AL_NB || i < 2) ? i : 3; t -= vec[a * NV + j] * misc[MI_XB + a]; }
            xv[j] = t;
        }
        __syncthreads();
        for (int j = n - 1; j >= 0; j--) {
            if (tid == 0) xv[j] = xv[j] / band[j * AL_BANDW + AL_BW];
            __syncthreads();
            if (tid >= 1 && tid <= AL_BW && j - tid >= 0) xv[j - tid] -= band[j * AL_BANDW + AL_BW - tid] * xv[j];
            __syncthreads();
        }
    };

    // ---- the velocity block: assembled (:168), x 1000 (:177), factored in place.  Entry (r, c): interval f - 1 first (its columns 3..5), then interval f
    build_records(false);
    for (int e = tid; e < n * AL_BANDW; e += AL_THREADS) {
        const int r = e / AL_BANDW, c = r - AL_BW + (e - AL_BANDW * r);
        double v = 0.0;
        if (c >= 0) {
            const int fr = r / 3, er = r - 3 * fr, fc = c / 3, ec = c - 3 * fc;
            if (fr == fc) {
                if (fr >= 1) v += al_rvv(rec + AL_REC * (fr - 1), 3 + er, 3 + ec);
                if (fr <= F - 2) v += al_rvv(rec + AL_REC * fr, er, ec);
            } else if (fr == fc + 1) v += al_rvv(rec + AL_REC * fc, 3 + er, ec);
            v *= 1000.0;
        }
        band[e] = v;
        if (c == r) diag0[r] = v;
    }
    __syncthreads();
    {
        // right-looking band Cholesky: column j's pivot behind the rank gate, lanes 1..5 scale the column, 15 lanes eliminate the 5 x 5 triangle
        int q = 0, p = 0;      // lane -> (q, p), 1 <= p <= q <= 5
        if (tid < 15) { int t = tid; q = 1; while (t >= q) { t -= q; q++; } p = t + 1; }
        double piv = 1.0;
        bool fail = false;
        for (int j = 0; j < n; j++) {
            const double d = band[j * AL_BANDW + AL_BW], a0 = diag0[j];
            if (!(d > opt.min_relative_pivot * a0)) { fail = true; break; }      // (uniform: every lane reads the same two numbers)
            piv = fmin(piv, d / a0);
            const double l = sqrt(d);
            __syncthreads();      // every lane has read the pivot
            if (tid == 0) band[j * AL_BANDW + AL_BW] = l;
            if (tid >= 1 && tid <= AL_BW && j + tid < n) band[(j + tid) * AL_BANDW + AL_BW - tid] = band[(j + tid) * AL_BANDW + AL_BW - tid] / l;
            __syncthreads();
            if (tid < 15 && j + q < n) band[(j + q) * AL_BANDW + AL_BW - (q - p)] -= band[(j + q) * AL_BANDW + AL_BW - q] * band[(j + p) * AL_BANDW + AL_BW - p];
            __syncthreads();
        }
        if (tid == 0) { misc[MI_PIV] = piv; if (fail) misc[MI_FAIL] = 1.0; }
        __syncthreads();
    }

    // level: what of the output record is filled -- 0 nothing, 1 scale and gravity_c0, 2 + velocity, 3 everything
    int status = 0, level = 0;
    double s = 0.0;
    V3 g;
    if (misc[MI_FAIL] != 0.0) status = 3;
    if (status == 0) {      // LinearAlignment
        assemble_vectors(0x1f);
        forward(0x1f);
        solve_border_and_back(AL_NB);
        if (misc[MI_FAIL] != 0.0) status = 3;
    }
    if (status == 0) {
        g = V3(misc[MI_XB], misc[MI_XB + 1], misc[MI_XB + 2]);
        s = misc[MI_XB + 3] / 100.0;                                             // :180
        level = 1;
        if (!al_finite(s) || !al_finite(g.x) || !al_finite(g.y) || !al_finite(g.z)) { status = 4; level = 0; }
        else if (fabs(sqrt(dot(g, g)) - G) > 1.0 || s < 0) status = 1;           // :184
    }
    if (status == 0) {      // RefineGravity
        V3 g0 = al_normalized(g) * G;                                            // :57
        for (int round = 0; round < 4 && status == 0; round++) {
            // TangentBasis (:40-53).  The reference tests a == tmp only; at a == -tmp its b is the zero vector, which its LDLT survives (zero
            // pivots give dg == 0) and a Cholesky behind a rank gate does not: both poles take the special branch here.
            const V3 a = al_normalized(g0);
            V3 tmp(0.0, 0.0, 1.0);
            if (a.x == tmp.x && a.y == tmp.y && (a.z == tmp.z || a.z == -tmp.z)) tmp = V3(1.0, 0.0, 0.0);
            const V3 lx = al_normalized(tmp - a * dot(a, tmp)), ly = cross(a, lx);
            __syncthreads();
            if (tid == 0) {
                misc[MI_G0] = g0.x; misc[MI_G0 + 1] = g0.y; misc[MI_G0 + 2] = g0.z;
                misc[MI_LX] = lx.x; misc[MI_LX + 1] = lx.y; misc[MI_LX + 2] = lx.z;
                misc[MI_LY] = ly.x; misc[MI_LY + 1] = ly.y; misc[MI_LY + 2] = ly.z;
            }
            __syncthreads();
            build_records(true);
            assemble_vectors(0x13);      // the two gravity rows and the right-hand side; the scale row's y is LinearAlignment's
            forward(0x13);
            solve_border_and_back(AL_NB - 1);
            if (misc[MI_FAIL] != 0.0) { status = 3; break; }
            const double dg0 = misc[MI_XB], dg1 = misc[MI_XB + 1];
            g0 = al_normalized(g0 + V3(lx.x * dg0 + ly.x * dg1, lx.y * dg0 + ly.y * dg1, lx.z * dg0 + ly.z * dg1)) * G;      // :119
        }
        if (status == 0) {
            g = g0;                                                              // :122
            s = misc[MI_XB + 3] / 100.0;                                         // :190
            level = 2;
            int bad = !al_finite(s) || !al_finite(g.x) || !al_finite(g.y) || !al_finite(g.z);
            for (int c = tid; c < n; c += AL_THREADS) bad |= !al_finite(xv[c]);
            if (__syncthreads_or(bad)) { status = 4; level = 0; }
            else if (s < 0.0) status = 2;                                        // :193
            else level = 3;
        } else level = 0;
    }
    __syncthreads();

    // ---- the output record; every entry is written once, zero where it was not computed
    M3 R0 = m3_zero();
    V3 g_w, P0;
    if (level == 3) {
        const M3 Rk0 = m3_load(R + 9 * key[0]);
        R0 = al_g2R(g);                                                          // estimator.cpp:1427
        double ypr[3];
        r2ypr(R0 * Rk0, ypr);                                                    // :1428
        R0 = ypr2R(-ypr[0], 0.0, 0.0) * R0;                                      // :1429
        g_w = R0 * g;                                                            // :1430
        P0 = s * V3(T + 3 * key[0]) - Rk0 * tic;
    }
    if (tid == 0) {
        O[0] = (double)status;
        O[1] = level >= 1 ? s : 0.0;
        O[2] = level >= 1 ? g.x : 0.0; O[3] = level >= 1 ? g.y : 0.0; O[4] = level >= 1 ? g.z : 0.0;
        O[5] = g_w.x; O[6] = g_w.y; O[7] = g_w.z;
        O[17] = misc[MI_PIV];
    }
    if (tid < 9) O[8 + tid] = R0.m[tid];
    if (tid >= 18 && tid < AL_HEAD) O[tid] = 0.0;
    for (int c = tid; c < n; c += AL_THREADS) O[AL_HEAD + c] = level >= 2 ? xv[c] : 0.0;
    double *oP = O + AL_HEAD + n, *oR = oP + 3 * K, *oV = oR + 9 * K;
    for (int kv = tid; kv < K; kv += AL_THREADS) {
        V3 Pk, Vk;
        M3 Rk = m3_zero();
        if (level == 3) {
            const int i = key[kv];
            const M3 Ri = m3_load(R + 9 * i);
            Pk = R0 * (s * V3(T + 3 * i) - Ri * tic - P0);                       // :1408, :1435
            Rk = R0 * Ri;                                                        // :1436
            Vk = R0 * (Ri * V3(xv[3 * kv], xv[3 * kv + 1], xv[3 * kv + 2]));     // :1416 (x indexed by kv), :1437
        }
        oP[3 * kv] = Pk.x; oP[3 * kv + 1] = Pk.y; oP[3 * kv + 2] = Pk.z;
        oV[3 * kv] = Vk.x; oV[3 * kv + 1] = Vk.y; oV[3 * kv + 2] = Vk.z;
#pragma unroll
        for (int e = 0; e < 9; e++) oR[9 * kv + e] = Rk.m[e];
    }
}

// solveGyroscopeBias (:3-27): per interval J = jacobian.block<3,3>(O_R, O_BG) and r = 2 vec(delta_q^-1 (x) q(Ri' Rj)); J'J and J'r summed in interval
// order; the 3 x 3 system by Cholesky behind the rank gate.  Dynamic LDS: 12 doubles per interval.
__global__ void __launch_bounds__(AL_THREADS) align_bias_kernel(int n_seq, const AlignHdr *hdrs, const double *Rg, const double *itv, double *out, double min_relative_pivot) {
    extern __shared__ __attribute__((aligned(16))) double al_lds_raw[];
    const int tid = threadIdx.x, seq = blockIdx.x;
    if (seq >= n_seq) return;
    const AlignHdr H = hdrs[seq];
    const int NI = H.n_frames - 1;
    lds_d *prod = (lds_d *)al_lds_raw, *sum = prod + 12 * NI;
    const double *R = Rg + 9 * (size_t)H.o_frame, *P = itv + (size_t)AL_BIAS_IN * H.o_itv;
    for (int i = tid; i < NI; i += AL_THREADS) {
        const M3 J = m3_load(P + AL_BIAS_IN * i);
        const Quat dq(P + AL_BIAS_IN * i + 9);
        const Quat q_ij = r2q(transpose(m3_load(R + 9 * i)) * m3_load(R + 9 * (i + 1)));      // :19
        const V3 r = 2.0 * (inverse(dq) * q_ij).vec();                                         // :21
        const M3 Jt = transpose(J), JtJ = Jt * J;                                              // :22
        const V3 Jtr = Jt * r;                                                                 // :23
#pragma unroll
        for (int e = 0; e < 9; e++) prod[12 * i + e] = JtJ.m[e];
        prod[12 * i + 9] = Jtr.x; prod[12 * i + 10] = Jtr.y; prod[12 * i + 11] = Jtr.z;
    }
    __syncthreads();
    if (tid < 12) {
        double s = 0.0;
        for (int i = 0; i < NI; i++) s += prod[12 * i + tid];
        sum[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double *o = out + (size_t)AL_BIAS_OUT * seq;
        const double a00 = sum[0], a10 = sum[3], a11 = sum[4], a20 = sum[6], a21 = sum[7], a22 = sum[8];
        double x0 = 0.0, x1 = 0.0, x2 = 0.0, piv = 1.0;
        int status = 3;
        do {
            const double d0 = a00;
            if (!(d0 > min_relative_pivot * a00)) break;
            const double l00 = sqrt(d0), l10 = a10 / l00, l20 = a20 / l00;
            const double d1 = a11 - l10 * l10;
            if (!(d1 > min_relative_pivot * a11)) break;
            const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
            const double d2 = a22 - l20 * l20 - l21 * l21;
            if (!(d2 > min_relative_pivot * a22)) break;
            const double l22 = sqrt(d2);
            piv = fmin(fmin(d0 / a00, d1 / a11), d2 / a22);
            const double y0 = sum[9] / l00, y1 = (sum[10] - l10 * y0) / l11, y2 = (sum[11] - l20 * y0 - l21 * y1) / l22;
            x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00;
            status = (al_finite(x0) && al_finite(x1) && al_finite(x2)) ? 0 : 4;
            if (status) x0 = x1 = x2 = 0.0;
        } while (0);
        o[0] = x0; o[1] = x1; o[2] = x2; o[3] = (double)status; o[4] = piv;
    }
}

}  // namespace tcv

extern "C" int tcv_launch_align_bias(int n, const tcv::AlignHdr *hdrs, const double *R, const double *itv, double *out, double min_relative_pivot, void *stream) {
    using namespace tcv;
    const size_t lds_bytes = sizeof(double) * (12 * (size_t)(128 - 1) + 16);      // TCV_VI_ALIGN_MAX_FRAMES intervals: 12 KB
    hipLaunchKernelGGL(align_bias_kernel, dim3(n), dim3(AL_THREADS), lds_bytes, (hipStream_t)stream, n, hdrs, R, itv, out, min_relative_pivot);
    return (int)hipGetLastError();
}
extern "C" int tcv_launch_align_solve(int n, const tcv::AlignHdr *hdrs, const double *R, const double *T, const double *itv, const int *keys, double *out,
                                      tcv::AlignOpts opts, size_t lds_bytes, void *stream) {
    using namespace tcv;
    hipError_t e = hipFuncSetAttribute((const void *)align_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(align_solve_kernel, dim3(n), dim3(AL_THREADS), lds_bytes, (hipStream_t)stream, n, hdrs, R, T, itv, keys, out, opts);
    return (int)hipGetLastError();
}
