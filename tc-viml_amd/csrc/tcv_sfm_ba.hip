// Batched bundle adjustment of the initial SfM (include/tcv_sfm_ba.h): the full BA of GlobalSFM::construct (reference
// initial_sfm.cpp:232-303) with Ceres' Levenberg-Marquardt loop restated on the device, one workgroup per problem.
//
// Linear algebra.  Unknowns: nc camera tangent columns (rotation 3, translation 3 per frame, the constant blocks left out), then 3 per point.
// Per linearisation every observation is evaluated once into its scratch record; per step
//   1. a thread per point: the damped 3 x 3 block H_pp = L L^T, y_p = L^-1 g_p and, per observation, Y = (J_c^T J_p) L^-T (6 x 3)
//   2. reduced camera system S = H_cc + D - sum_p Y_p Y_p^T, right-hand side g_c - sum_p Y_p y_p as one more row: a thread owns a 4 x 4 tile
//      of the lower triangle in registers; the zero-padded Y of BA_CHUNK points at a time is staged in LDS, points and rows ascending
//   3. dense Cholesky of S in LDS, the right-hand side riding as row nc; back substitution of the cameras, then of the points
// Every sum has one fixed order and no atomics: the same bits from run to run and in any batch.  FP64 throughout.  All LDS is dynamic.
// The host has validated every index: nothing here checks a bound to stay inside its buffers.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "tcv_sfm_ba.h"

namespace tcv {

struct BaCtx {
    int F, P, NO, nc, ncp;
    const int *ofr, *opt, *pfirst, *fptr, *fobs, *coff, *colinfo;
    const double *uv;
    double *x, *xc, *scale, *delta, *rec, *ptrec;      // global scratch
    double *red, *S, *chunk, *Hc, *dinv, *ys;           // LDS
    BaOpts o;
};

// sum over the workgroup in one fixed order (tree over the 256 lanes); every thread gets the result
__device__ double ba_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = BA_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}
__device__ double ba_block_max(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = BA_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);      // (fmax drops a NaN: the callers turn non-finite values into a flag first)
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ bool ba_finite(double v) { return fabs(v) < 1e300; }

// cost at `x`; with `jac` the records of the linearisation (J_camera | r | J_point, unscaled).  *ok: every residual is finite
__device__ double ba_eval(const BaCtx &c, const double *x, bool jac, bool *ok) {
    double s = 0.0, bad = 0.0;
    for (int o = threadIdx.x; o < c.NO; o += BA_THREADS) {
        const int f = c.ofr[o], p = c.opt[o];
        double r[2], Jc[12], Jp[6];
        const double v = ba_observation(x + 4 * f, x + 4 * c.F + 3 * f, x + 7 * c.F + 3 * p, c.uv + 2 * o, r, jac ? Jc : nullptr, jac ? Jp : nullptr);
        if (!ba_finite(v)) bad = 1.0;
        s += v;
        if (jac) {
            double *R = c.rec + (size_t)BA_REC * o;
            for (int k = 0; k < 12; k++) R[k] = Jc[k];
            R[12] = r[0]; R[13] = r[1];
            for (int k = 0; k < 6; k++) R[14 + k] = Jp[k];
        }
    }
    *ok = ba_block_max(bad, c.red) == 0.0;
    return ba_block_sum(s, c.red);      // (ends in a barrier: the records are visible)
}

// per frame the lower triangle of its 6 x 6 block of J^T J and its 6 entries of J^T r (unscaled), over the frame's observations ascending
__device__ void ba_frame_pass(const BaCtx &c) {
    for (int i = threadIdx.x; i < BA_HC * c.F; i += BA_THREADS) {
        const int f = i / BA_HC, e = i % BA_HC;
        int a = 0, b;
        if (e < 21) { while ((a + 1) * (a + 2) / 2 <= e) a++; b = e - a * (a + 1) / 2; }
        else { a = e - 21; b = 12; }      // (column 12, 13 of a record's rows: the residual)
        double v = 0.0;
        for (int q = c.fptr[f]; q < c.fptr[f + 1]; q++) {
            const double *R = c.rec + (size_t)BA_REC * c.fobs[q];
            const double rb0 = e < 21 ? R[b] : R[12], rb1 = e < 21 ? R[6 + b] : R[13];
            v += R[a] * rb0 + R[6 + a] * rb1;
        }
        c.Hc[i] = v;
    }
    __syncthreads();
}
// mode 0: scale = 1 / (1 + ||column of J||) over every column (Jacobi scaling, iteration 0); mode 1: max |J^T r| of the unscaled Jacobian
__device__ double ba_column_pass(const BaCtx &c, int mode) {
    double gmax = 0.0;
    for (int j = threadIdx.x; j < c.nc; j += BA_THREADS) {
        const int f = c.colinfo[j] / 6, k = c.colinfo[j] % 6;
        if (mode == 0) c.scale[j] = 1.0 / (1.0 + sqrt(c.Hc[BA_HC * f + k * (k + 1) / 2 + k]));
        else gmax = fmax(gmax, fabs(c.Hc[BA_HC * f + 21 + k]));
    }
    for (int p = threadIdx.x; p < c.P; p += BA_THREADS) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int o = c.pfirst[p]; o < c.pfirst[p + 1]; o++) {
            const double *R = c.rec + (size_t)BA_REC * o;
            for (int m = 0; m < 3; m++) acc[m] += mode == 0 ? R[14 + m] * R[14 + m] + R[17 + m] * R[17 + m] : R[14 + m] * R[12] + R[17 + m] * R[13];
        }
        for (int m = 0; m < 3; m++) {
            if (mode == 0) c.scale[c.nc + 3 * p + m] = 1.0 / (1.0 + sqrt(acc[m]));
            else gmax = fmax(gmax, fabs(acc[m]));
        }
    }
    return mode == 0 ? 0.0 : ba_block_max(gmax, c.red);
}

// the damped normal equations of the Jacobi-scaled Jacobian solved exactly; c.delta = -scale * y.  false: a pivot was not positive or the
// step is not finite
__device__ bool ba_solve(const BaCtx &c, double radius) {
    const int t = threadIdx.x, nc = c.nc, ncp = c.ncp;
    // 1. points: H_pp + D = L L^T, y_p = L^-1 g_p, Y of every observation
    double bad = 0.0;
    for (int p = t; p < c.P; p += BA_THREADS) {
        const double *sp = c.scale + nc + 3 * p;
        double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};      // 00 10 11 20 21 22
        for (int o = c.pfirst[p]; o < c.pfirst[p + 1]; o++) {
            const double *R = c.rec + (size_t)BA_REC * o;
            for (int row = 0; row < 2; row++) {
                const double j0 = R[14 + 3 * row] * sp[0], j1 = R[15 + 3 * row] * sp[1], j2 = R[16 + 3 * row] * sp[2], r = R[12 + row];
                H[0] += j0 * j0; H[1] += j1 * j0; H[2] += j1 * j1; H[3] += j2 * j0; H[4] += j2 * j1; H[5] += j2 * j2;
                g[0] += j0 * r; g[1] += j1 * r; g[2] += j2 * r;
            }
        }
        // LevenbergMarquardtStrategy::ComputeStep: D = sqrt(clamp(diag(J^T J)) / radius), the system gets D^2
        for (int m = 0; m < 3; m++) {
            const int d = m * (m + 1) / 2 + m;
            const double l = sqrt(fmin(fmax(H[d], 1e-6), 1e32) / radius);
            H[d] += l * l;
        }
        double L[6], il[3];
        bool ok = H[0] > 0.0 && H[0] < 1e300;
        L[0] = sqrt(H[0]); il[0] = 1.0 / L[0];
        L[1] = H[1] * il[0]; L[3] = H[3] * il[0];
        const double d1 = H[2] - L[1] * L[1];
        ok = ok && d1 > 0.0 && d1 < 1e300;
        L[2] = sqrt(d1); il[1] = 1.0 / L[2];
        L[4] = (H[4] - L[3] * L[1]) * il[1];
        const double d2 = H[5] - L[3] * L[3] - L[4] * L[4];
        ok = ok && d2 > 0.0 && d2 < 1e300;
        L[5] = sqrt(d2); il[2] = 1.0 / L[5];
        if (!ok) { bad = 1.0; continue; }
        double *PR = c.ptrec + (size_t)BA_PT * p;
        for (int k = 0; k < 6; k++) PR[k] = L[k];
        const double y0 = g[0] * il[0], y1 = (g[1] - L[1] * y0) * il[1], y2 = (g[2] - L[3] * y0 - L[4] * y1) * il[2];
        PR[6] = y0; PR[7] = y1; PR[8] = y2;
        for (int o = c.pfirst[p]; o < c.pfirst[p + 1]; o++) {
            double *R = c.rec + (size_t)BA_REC * o;
            const int f = c.ofr[o];
            double js[6];
            for (int row = 0; row < 2; row++)
                for (int m = 0; m < 3; m++) js[3 * row + m] = R[14 + 3 * row + m] * sp[m];
            for (int i = 0; i < 6; i++) {
                const int col = c.coff[2 * f + i / 3];
                const double sc = col >= 0 ? c.scale[col + i % 3] : 0.0;      // (a constant block: zeros nobody reads)
                const double a0 = R[i] * sc, a1 = R[6 + i] * sc;
                const double w0 = a0 * js[0] + a1 * js[3], w1 = a0 * js[1] + a1 * js[4], w2 = a0 * js[2] + a1 * js[5];
                const double v0 = w0 * il[0], v1 = (w1 - v0 * L[1]) * il[1], v2 = (w2 - v0 * L[3] - v1 * L[4]) * il[2];      // W L^-T
                R[20 + 3 * i] = v0; R[21 + 3 * i] = v1; R[22 + 3 * i] = v2;
            }
        }
    }
    if (ba_block_max(bad, c.red) != 0.0) return false;
    // 2. the thread's tile of sum_p Y_p Y_p^T (row and column nc: sum_p Y_p y_p), chunk by chunk, rows ascending
    const int ntile = ncp / BA_TILE;
    int ti = -1, tj = 0;
    {
        int q = t;
        for (int a = 0; a < ntile; a++) { if (q <= a) { ti = a; tj = q; break; } q -= a + 1; }
    }
    double acc[BA_TILE * BA_TILE];
    for (int i = 0; i < BA_TILE * BA_TILE; i++) acc[i] = 0.0;
    for (int p0 = 0; p0 < c.P; p0 += BA_CHUNK) {
        const int np = min((int)BA_CHUNK, c.P - p0), o0 = c.pfirst[p0], o1 = c.pfirst[p0 + np];
        __syncthreads();
        for (int i = t; i < 3 * BA_CHUNK * ncp; i += BA_THREADS) c.chunk[i] = 0.0;
        __syncthreads();
        for (int i = t; i < 18 * (o1 - o0); i += BA_THREADS) {
            const int o = o0 + i / 18, e = i % 18, f = c.ofr[o], col = c.coff[2 * f + e / 9];
            if (col >= 0) c.chunk[(3 * (c.opt[o] - p0) + e % 3) * ncp + col + (e / 3) % 3] = c.rec[(size_t)BA_REC * o + 20 + e];
        }
        for (int i = t; i < 3 * np; i += BA_THREADS) c.chunk[i * ncp + nc] = c.ptrec[(size_t)BA_PT * (p0 + i / 3) + 6 + i % 3];
        __syncthreads();
        if (ti >= 0) {
            const double *A = c.chunk + BA_TILE * ti, *B = c.chunk + BA_TILE * tj;
            for (int k = 0; k < 3 * np; k++) {
                double a[BA_TILE], b[BA_TILE];
                for (int i = 0; i < BA_TILE; i++) { a[i] = A[k * ncp + i]; b[i] = B[k * ncp + i]; }
                for (int i = 0; i < BA_TILE; i++)
                    for (int j = 0; j < BA_TILE; j++) acc[BA_TILE * i + j] += a[i] * b[j];
            }
        }
    }
    // S = H_cc + D - the tile; H_cc is block diagonal (no residual sees two cameras)
    if (ti >= 0) {
        for (int i = 0; i < BA_TILE; i++)
            for (int j = 0; j < BA_TILE; j++) {
                const int r = BA_TILE * ti + i, cc = BA_TILE * tj + j;
                if (r > nc || cc >= nc || cc > r) continue;
                const int fc = c.colinfo[cc] / 6, kc = c.colinfo[cc] % 6;
                double base = 0.0;
                if (r == nc) base = c.scale[cc] * c.Hc[BA_HC * fc + 21 + kc];
                else {
                    const int fr = c.colinfo[r] / 6, kr = c.colinfo[r] % 6;
                    if (fr == fc) base = c.scale[r] * c.scale[cc] * c.Hc[BA_HC * fc + kr * (kr + 1) / 2 + kc];
                    if (r == cc) {
                        const double l = sqrt(fmin(fmax(base, 1e-6), 1e32) / radius);
                        base += l * l;
                    }
                }
                c.S[r * ncp + cc] = base - acc[BA_TILE * i + j];
            }
    }
    __syncthreads();
    // 3. dense Cholesky, right-looking, in place; row nc becomes z = L^-1 (right-hand side)
    bool ok = true;
    for (int k = 0; k < nc; k++) {
        const double piv = c.S[k * ncp + k];
        if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }      // (the same value in every thread: uniform)
        const double inv = 1.0 / sqrt(piv);
        for (int r = k + 1 + t; r <= nc; r += BA_THREADS) c.S[r * ncp + k] *= inv;
        if (t == 0) c.dinv[k] = inv;
        __syncthreads();
        const int n = nc - k;      // rows k + 1 .. nc; row nc has no diagonal entry
        for (int i = t; i < n * n; i += BA_THREADS) {
            const int r = k + 1 + i / n, cc = k + 1 + i % n;
            if (cc <= r && cc < nc) c.S[r * ncp + cc] -= c.S[r * ncp + k] * c.S[cc * ncp + k];
        }
        __syncthreads();
    }
    if (!ok) { __syncthreads(); return false; }
    // back substitution L^T ys = z, z updated in place, one column per barrier
    for (int k = nc - 1; k >= 0; k--) {
        const double xk = c.S[nc * ncp + k] * c.dinv[k];
        if (t == 0) c.ys[k] = xk;
        for (int j = t; j < k; j += BA_THREADS) c.S[nc * ncp + j] -= c.S[k * ncp + j] * xk;
        __syncthreads();
    }
    // points: L^T y = y_p - Y_p^T ys
    bad = 0.0;
    for (int j = t; j < nc; j += BA_THREADS) {
        const double d = -c.scale[j] * c.ys[j];
        c.delta[j] = d;
        if (!ba_finite(d)) bad = 1.0;
    }
    for (int p = t; p < c.P; p += BA_THREADS) {
        const double *PR = c.ptrec + (size_t)BA_PT * p;
        double v[3] = {PR[6], PR[7], PR[8]};
        for (int o = c.pfirst[p]; o < c.pfirst[p + 1]; o++) {
            const double *R = c.rec + (size_t)BA_REC * o;
            const int f = c.ofr[o];
            for (int i = 0; i < 6; i++) {
                const int col = c.coff[2 * f + i / 3];
                if (col < 0) continue;
                const double yc = c.ys[col + i % 3];
                for (int m = 0; m < 3; m++) v[m] -= R[20 + 3 * i + m] * yc;
            }
        }
        const double y2 = v[2] / PR[5], y1 = (v[1] - PR[4] * y2) / PR[2], y0 = (v[0] - PR[1] * y1 - PR[3] * y2) / PR[0];
        const double y[3] = {y0, y1, y2};
        for (int m = 0; m < 3; m++) {
            const double d = -c.scale[nc + 3 * p + m] * y[m];
            c.delta[nc + 3 * p + m] = d;
            if (!ba_finite(d)) bad = 1.0;
        }
    }
    return ba_block_max(bad, c.red) == 0.0;      // (ends in a barrier: delta is visible)
}

// -(J d) . (r + J d / 2) over the observations, d = c.delta (TrustRegionMinimizer: model_cost_change)
__device__ double ba_model_cost_change(const BaCtx &c) {
    double s = 0.0;
    for (int o = threadIdx.x; o < c.NO; o += BA_THREADS) {
        const double *R = c.rec + (size_t)BA_REC * o;
        const int f = c.ofr[o], p = c.opt[o];
        for (int row = 0; row < 2; row++) {
            double jd = 0.0;
            for (int i = 0; i < 6; i++) {
                const int col = c.coff[2 * f + i / 3];
                if (col >= 0) jd += R[6 * row + i] * c.delta[col + i % 3];
            }
            for (int m = 0; m < 3; m++) jd += R[14 + 3 * row + m] * c.delta[c.nc + 3 * p + m];
            s -= jd * (R[12 + row] + 0.5 * jd);
        }
    }
    return ba_block_sum(s, c.red);
}

// c.xc = Plus(c.x, c.delta): ceres::QuaternionParameterization for the rotations, nothing renormalised; constant blocks are copied.
// dx2, x2: squared norms of the step and of x over the ambient coordinates of the non-constant blocks
__device__ void ba_plus(const BaCtx &c, double *dx2_out, double *x2_out) {
    double dx2 = 0.0, x2 = 0.0;
    for (int b = threadIdx.x; b < 2 * c.F + c.P; b += BA_THREADS) {
        int off, n, col;
        if (b < c.F) { off = 4 * b; n = 4; col = c.coff[2 * b]; }
        else if (b < 2 * c.F) { off = 4 * c.F + 3 * (b - c.F); n = 3; col = c.coff[2 * (b - c.F) + 1]; }
        else { off = 7 * c.F + 3 * (b - 2 * c.F); n = 3; col = c.nc + 3 * (b - 2 * c.F); }
        const double *x = c.x + off;
        double v[4] = {x[0], x[1], x[2], n == 4 ? x[3] : 0.0};
        if (col >= 0) {
            const double *d = c.delta + col;
            if (n == 4) {
                const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (nd > 0.0) {
                    const double k = sin(nd) / nd, q0 = cos(nd), q1 = k * d[0], q2 = k * d[1], q3 = k * d[2];      // QuaternionProduct(q_delta, x)
                    v[0] = q0 * x[0] - q1 * x[1] - q2 * x[2] - q3 * x[3];
                    v[1] = q0 * x[1] + q1 * x[0] + q2 * x[3] - q3 * x[2];
                    v[2] = q0 * x[2] - q1 * x[3] + q2 * x[0] + q3 * x[1];
                    v[3] = q0 * x[3] + q1 * x[2] - q2 * x[1] + q3 * x[0];
                }
            } else {
                for (int k = 0; k < 3; k++) v[k] = x[k] + d[k];
            }
            for (int k = 0; k < n; k++) { dx2 += (v[k] - x[k]) * (v[k] - x[k]); x2 += x[k] * x[k]; }
        }
        for (int k = 0; k < n; k++) c.xc[off + k] = v[k];
    }
    *dx2_out = ba_block_sum(dx2, c.red);
    *x2_out = ba_block_sum(x2, c.red);
}

extern __shared__ __attribute__((aligned(16))) double ba_lds[];

__global__ void __launch_bounds__(BA_THREADS) sfm_ba_kernel(int n_problems, const BaHdr *hdrs, const int *ipool, const double *dpool, double *scratch,
                                                            double *out, BaOpts opts) {
    const int g = blockIdx.x, t = threadIdx.x;
    if (g >= n_problems) return;
    const BaHdr H = hdrs[g];
    BaCtx c;
    c.F = H.n_frames; c.P = H.n_points; c.NO = H.n_obs; c.nc = H.nc; c.ncp = (H.nc + 1 + BA_TILE - 1) / BA_TILE * BA_TILE;
    const int *ip = ipool + H.o_int;
    c.ofr = ip; c.opt = c.ofr + c.NO; c.pfirst = c.opt + c.NO; c.fptr = c.pfirst + c.P + 1; c.fobs = c.fptr + c.F + 1; c.coff = c.fobs + c.NO;
    c.colinfo = c.coff + 2 * c.F;
    const int nx = 7 * c.F + 3 * c.P, nu = c.nc + 3 * c.P;
    const double *xin = dpool + H.o_dbl;
    c.uv = xin + nx;
    double *s = scratch + H.o_scr;
    c.x = s; c.xc = c.x + nx; c.scale = c.xc + nx; c.delta = c.scale + nu; c.rec = c.delta + nu; c.ptrec = c.rec + (size_t)BA_REC * c.NO;
    c.red = ba_lds; c.S = c.red + BA_THREADS; c.chunk = c.S + c.ncp * c.ncp; c.Hc = c.chunk + 3 * BA_CHUNK * c.ncp; c.dinv = c.Hc + BA_HC * c.F;
    c.ys = c.dinv + c.ncp;
    c.o = opts;
    double *o_x = out + H.o_out, *o_sum = o_x + nx;

    for (int i = t; i < nx; i += BA_THREADS) c.x[i] = xin[i];
    for (int i = t; i < BA_SUM; i += BA_THREADS) o_sum[i] = 0.0;
    __syncthreads();

    // ---- TrustRegionMinimizer with LevenbergMarquardtStrategy
    int n_rec = 0, termination = 0;
    auto record = [&](double cst, double cand, double rho, double radius, int step) {
        if (t == 0 && n_rec < BA_T) {
            o_sum[4 + n_rec] = cst; o_sum[4 + BA_T + n_rec] = cand; o_sum[4 + 2 * BA_T + n_rec] = rho; o_sum[4 + 3 * BA_T + n_rec] = radius;
            o_sum[4 + 4 * BA_T + n_rec] = (double)step;
        }
        n_rec++;
    };
    bool finite = true;
    double cost = ba_eval(c, c.x, true, &finite);
    double initial_cost = cost;
    bool done = false;
    if (!finite) { termination = 5; done = true; cost = initial_cost = DBL_MAX; }      // the initial evaluation failed: no record, the state as given
    else record(cost, 0.0, 0.0, opts.radius0, 1);
    if (!done) {
        ba_frame_pass(c);
        ba_column_pass(c, 0);
        __syncthreads();
        if (ba_column_pass(c, 1) <= opts.gtol) { termination = 1; done = true; }
    }
    double radius = opts.radius0, decrease_factor = 2.0;
    int invalid = 0, iter = 0;
    while (!done) {
        if (iter >= opts.max_it) { termination = 0; break; }
        if (radius < 1e-32) { termination = 4; break; }
        iter++;
        bool valid = ba_solve(c, radius);
        double mcc = 0.0;
        if (valid) { mcc = ba_model_cost_change(c); valid = mcc > 0.0; }
        if (!valid) {
            record(cost, 0.0, 0.0, radius, -1);
            if (++invalid >= opts.max_invalid) { termination = 5; break; }
            radius *= 0.5;      // LevenbergMarquardtStrategy::StepIsInvalid
            continue;
        }
        invalid = 0;
        double dx2, x2;
        ba_plus(c, &dx2, &x2);
        bool cand_ok;
        double cand = ba_eval(c, c.xc, false, &cand_ok);
        if (!cand_ok) cand = DBL_MAX;      // ComputeCandidatePointAndEvaluateCost: a candidate that cannot be evaluated is a rejected step
        const double cost_change = cost - cand, rho = cost_change / mcc;
        if (sqrt(dx2) <= opts.ptol * (sqrt(x2) + opts.ptol)) { record(cost, cand, rho, radius, 0); termination = 2; break; }
        if (fabs(cost_change) <= opts.ftol * cost) { record(cost, cand, rho, radius, 0); termination = 3; break; }
        if (rho > opts.min_rel_dec) {
            for (int i = t; i < nx; i += BA_THREADS) c.x[i] = c.xc[i];
            __syncthreads();
            bool ok_again;
            (void)ba_eval(c, c.x, true, &ok_again);      // the next linearisation: every observation once
            cost = cand;
            record(cost, cand, rho, radius, 1);
            const double q = 2.0 * rho - 1.0;      // LevenbergMarquardtStrategy::StepAccepted
            radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
            decrease_factor = 2.0;
            ba_frame_pass(c);
            if (ba_column_pass(c, 1) <= opts.gtol) { termination = 1; break; }
        } else {
            record(cost, cand, rho, radius, 0);
            radius /= decrease_factor;      // StepRejected
            decrease_factor *= 2.0;
        }
    }
    __syncthreads();
    // after FAILURE x still holds the last accepted state: never a NaN
    for (int i = t; i < nx; i += BA_THREADS) o_x[i] = c.x[i];
    if (t == 0) { o_sum[0] = initial_cost; o_sum[1] = cost; o_sum[2] = (double)n_rec; o_sum[3] = (double)termination; }
}

// n independent observations: in = [q 4 | t 3 | X 3 | uv 2], out = [r 2 | J 2 x 9 | cost]
__global__ void __launch_bounds__(64) sfm_ba_observations_kernel(int n, const double *in, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *e = in + (size_t)BA_OBS_IN * i;
    double r[2], Jc[12], Jp[6];
    const double cost = ba_observation(e, e + 4, e + 7, e + 10, r, Jc, Jp);
    double *o = out + (size_t)BA_OBS_OUT * i;
    o[0] = r[0]; o[1] = r[1];
    for (int row = 0; row < 2; row++) {
        for (int k = 0; k < 6; k++) o[2 + 9 * row + k] = Jc[6 * row + k];
        for (int k = 0; k < 3; k++) o[2 + 9 * row + 6 + k] = Jp[3 * row + k];
    }
    o[20] = cost;
}

}  // namespace tcv

extern "C" int tcv_launch_sfm_ba(int n, const tcv::BaHdr *hdrs, const int *ipool, const double *dpool, double *scratch, double *out, tcv::BaOpts opts,
                                 size_t lds_bytes, void *stream) {
    using namespace tcv;
    hipError_t e = hipFuncSetAttribute((const void *)sfm_ba_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sfm_ba_kernel, dim3(n), dim3(BA_THREADS), lds_bytes, (hipStream_t)stream, n, hdrs, ipool, dpool, scratch, out, opts);
    return (int)hipGetLastError();
}
extern "C" int tcv_launch_sfm_ba_observations(int n, const double *in, double *out, void *stream) {
    using namespace tcv;
    hipLaunchKernelGGL(sfm_ba_observations_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, in, out);
    return (int)hipGetLastError();
}
