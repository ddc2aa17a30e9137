// Batched 4-DoF pose-graph optimisation (include/tcv_pose_graph.h): PoseGraph::optimize4DoF of the reference
// (pose_graph/src/pose_graph.cpp:403-579) with Ceres' Levenberg-Marquardt loop restated on the device, one workgroup per graph.
//
// Linear algebra.  Unknowns are 4 per free node (yaw, t).  The host orders the free nodes: first, in keyframe order, every node that is
// not the newer end of a loop edge with a free older end (the BAND: sequence edges reach four nodes back, so the normal matrix of these
// nodes has a scalar half-bandwidth of PG_BW = 19, and taking nodes out only shortens distances); then the newer ends (the BORDER, dense).
//   1. band Cholesky, right-looking, one column per barrier, on panels of the band staged in LDS           (serial: n_band columns)
//   2. forward substitution of the border rows and of the right-hand side through the band factor          (one thread per row)
//   3. Schur complement of the border (4 x 4 register tiles), dense Cholesky of it, right-hand side as one more row
//   4. back substitution: border, then band
// Every sum has one fixed order and no atomics: the same bits from run to run and in any batch.  FP64 throughout.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tcv_pose_graph.h"
#include "tcv_host.h"
#include "tcv_pose_graph.h"

namespace tcv {

enum { PG_THREADS = 256, PG_PANEL_ROWS = 320, PG_PANEL_COLS = PG_PANEL_ROWS - PG_BW, PG_MAX_INVALID = 5, PG_KC = 32 };
// the output record of one graph behind its poses: [initial_cost, final_cost, yaw_drift, r_drift 9, t_drift 3 | cost, cost_candidate, rho,
// radius: MAX_TRACE each | iterations, termination, step MAX_TRACE (integers as doubles)]
enum { PG_T = TCV_POSE_GRAPH_MAX_TRACE, PG_SUM = 15 + 4 * PG_T + 2 + PG_T };

struct PgHdr {
    int n_nodes, n_free, nb, nk, n_edges, n_loops, pad0_, pad1_;
    long long o_int, o_dbl, o_scr, o_out;      // this graph's ints (in ints), input doubles, scratch doubles, output doubles
};
// scratch of one graph, in doubles (the host sizes it, the kernel walks it the same way)
struct PgScratch {
    long long ypr, x, xc, meas, scale, delta, dinv, xs, tvec, AB, W, S, total;
    __host__ __device__ PgScratch(int N, int F, int nb, int nk, int E) {
        const long long nbs = 4LL * nb, M1 = 4LL * nk + 1;
        long long o = 0;
        ypr = o; o += 3LL * N; x = o; o += 4LL * N; xc = o; o += 4LL * N; meas = o; o += 6LL * E;
        scale = o; o += 4LL * F + 4; delta = o; o += 4LL * F + 4; dinv = o; o += M1; xs = o; o += M1; tvec = o; o += nbs + 4;
        AB = o; o += PG_LD * (nbs + PG_LD); W = o; o += M1 * nbs; S = o; o += M1 * M1;
        total = o;
    }
};

struct PgCtx {
    int N, F, nb, nk, E, nbs, m, M1;
    const int *pos, *ea, *eb, *ek, *cptr, *cent, *nodeof;
    double *ypr, *x, *xc, *meas, *scale, *delta, *dinv, *xs, *tvec, *AB, *W, *S;
    PgOpts o;
    double *red, *panel, *dinv_band;
};

// sum over the workgroup in one fixed order (tree over the 256 lanes); every thread gets the result
__device__ double pg_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}
__device__ double pg_block_max(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = PG_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);      // (fmax drops a NaN: the callers test for non-finite values separately)
        __syncthreads();
    }
    return red[0];
}

// cost of the reduced problem at `x` (edges with a free end) and, optionally, of the edges between two constant nodes
__device__ double pg_cost(const PgCtx &c, const double *x, double *fixed_cost) {
    double s = 0.0, f = 0.0;
    for (int e = threadIdx.x; e < c.E; e += PG_THREADS) {
        const int a = c.ea[e], b = c.eb[e];
        const double v = pg_edge(c.ek[e] != 0, x + 4 * a, x + 4 * b, c.meas + 6 * e, c.o, false, nullptr, nullptr, nullptr);
        if (c.pos[a] < 0 && c.pos[b] < 0) f += v; else s += v;
    }
    s = pg_block_sum(s, c.red);
    if (fixed_cost) *fixed_cost = pg_block_sum(f, c.red);
    return s;
}
// -(J d) . (r + J d / 2) over the edges of the reduced problem, d = c.delta (TrustRegionMinimizer: model_cost_change)
__device__ double pg_model_cost_change(const PgCtx &c) {
    double s = 0.0;
    for (int e = threadIdx.x; e < c.E; e += PG_THREADS) {
        const int a = c.ea[e], b = c.eb[e], pa = c.pos[a], pb = c.pos[b];
        if (pa < 0 && pb < 0) continue;
        double r[4], Ja[16], Jb[16];
        pg_edge(c.ek[e] != 0, c.x + 4 * a, c.x + 4 * b, c.meas + 6 * e, c.o, true, r, Ja, Jb);
        for (int row = 0; row < 4; row++) {
            double jd = 0.0;
            if (pa >= 0) for (int k = 0; k < 4; k++) jd += Ja[4 * row + k] * c.delta[4 * pa + k];
            if (pb >= 0) for (int k = 0; k < 4; k++) jd += Jb[4 * row + k] * c.delta[4 * pb + k];
            s -= jd * (r[row] + 0.5 * jd);
        }
    }
    return pg_block_sum(s, c.red);
}
// one thread per free node over its incident edges.  mode 0: scale = 1 / (1 + ||column of J||) (Jacobi scaling, iteration 0);
// mode 1: returns max |J^T r| of the unscaled Jacobian (gradient_max_norm)
__device__ double pg_node_pass(const PgCtx &c, int mode) {
    double gmax = 0.0;
    for (int p = threadIdx.x; p < c.F; p += PG_THREADS) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int q = c.cptr[p]; q < c.cptr[p + 1]; q++) {
            const int e = c.cent[q] >> 1, side = c.cent[q] & 1;
            double r[4], Ja[16], Jb[16];
            pg_edge(c.ek[e] != 0, c.x + 4 * c.ea[e], c.x + 4 * c.eb[e], c.meas + 6 * e, c.o, true, r, Ja, Jb);
            const double *J = side ? Jb : Ja;
            for (int k = 0; k < 4; k++)
                for (int row = 0; row < 4; row++) acc[k] += mode == 0 ? J[4 * row + k] * J[4 * row + k] : J[4 * row + k] * r[row];
        }
        for (int k = 0; k < 4; k++) {
            if (mode == 0) c.scale[4 * p + k] = 1.0 / (1.0 + sqrt(acc[k]));
            else gmax = fmax(gmax, fabs(acc[k]));
        }
    }
    return mode == 0 ? 0.0 : pg_block_max(gmax, c.red);
}

// where entry (row, col <= row) of the ordered, scaled normal matrix lives
__device__ __forceinline__ double *pg_entry(const PgCtx &c, int row, int col) {
    if (row < c.nbs) return c.AB + (size_t)row * PG_LD + (row - col);
    const int r = row - c.nbs;
    return col < c.nbs ? c.W + (size_t)col * c.M1 + r : c.S + (size_t)r * c.M1 + (col - c.nbs);
}
// J^T J and J^T r of the Jacobi-scaled Jacobian at c.x, plus the LM diagonal: the thread of a node owns the node's four rows
__device__ void pg_assemble(const PgCtx &c, double radius) {
    const int t = threadIdx.x;
    __syncthreads();
    for (size_t i = t; i < (size_t)PG_LD * c.nbs; i += PG_THREADS) c.AB[i] = 0.0;
    for (size_t i = t; i < (size_t)c.M1 * c.nbs; i += PG_THREADS) c.W[i] = 0.0;
    for (size_t i = t; i < (size_t)c.M1 * c.M1; i += PG_THREADS) c.S[i] = 0.0;
    __syncthreads();
    for (int p = t; p < c.F; p += PG_THREADS) {
        double g[4] = {0.0, 0.0, 0.0, 0.0}, D[16];
        for (int k = 0; k < 16; k++) D[k] = 0.0;
        for (int q = c.cptr[p]; q < c.cptr[p + 1]; q++) {
            const int e = c.cent[q] >> 1, side = c.cent[q] & 1;
            const int a = c.ea[e], b = c.eb[e];
            double r[4], Ja[16], Jb[16];
            pg_edge(c.ek[e] != 0, c.x + 4 * a, c.x + 4 * b, c.meas + 6 * e, c.o, true, r, Ja, Jb);
            double *Jm = side ? Jb : Ja, *Jo = side ? Ja : Jb;
            const int po = c.pos[side ? a : b];
            for (int k = 0; k < 4; k++)
                for (int row = 0; row < 4; row++) Jm[4 * row + k] *= c.scale[4 * p + k];
            for (int k = 0; k < 4; k++)
                for (int row = 0; row < 4; row++) g[k] += Jm[4 * row + k] * r[row];
            for (int k1 = 0; k1 < 4; k1++)
                for (int k2 = 0; k2 <= k1; k2++)
                    for (int row = 0; row < 4; row++) D[4 * k1 + k2] += Jm[4 * row + k1] * Jm[4 * row + k2];
            if (po >= 0 && po < p) {
                for (int k1 = 0; k1 < 4; k1++)
                    for (int k2 = 0; k2 < 4; k2++) {
                        double v = 0.0;
                        for (int row = 0; row < 4; row++) v += Jm[4 * row + k1] * (Jo[4 * row + k2] * c.scale[4 * po + k2]);
                        *pg_entry(c, 4 * p + k1, 4 * po + k2) += v;
                    }
            }
        }
        for (int k1 = 0; k1 < 4; k1++) {
            // LevenbergMarquardtStrategy::ComputeStep: D = sqrt(clamp(diag(J^T J)) / radius), the system gets D^2
            const double d = fmin(fmax(D[4 * k1 + k1], 1e-6), 1e32), l = sqrt(d / radius);
            D[4 * k1 + k1] += l * l;
            for (int k2 = 0; k2 <= k1; k2++) *pg_entry(c, 4 * p + k1, 4 * p + k2) = D[4 * k1 + k2];
            const int row = 4 * p + k1;
            if (row < c.nbs) c.W[(size_t)row * c.M1 + c.m] = g[k1];      // the right-hand side is row m of the border
            else c.S[(size_t)c.m * c.M1 + (row - c.nbs)] = g[k1];
        }
    }
    __syncthreads();
}

// the damped normal equations solved exactly; c.delta = -scale * y.  false: a pivot was not positive or the step is not finite
__device__ bool pg_solve(const PgCtx &c, int d1, int d2) {
    const int t = threadIdx.x, nbs = c.nbs, m = c.m, M1 = c.M1;
    // 1. band Cholesky, in place, in LDS: afterwards AB[k][0] = 1 / L_kk, AB[k][d] = L[k][k - d]; no global store inside the column loop
    bool ok = true;
    for (int k0 = 0; k0 < nbs && ok; k0 += PG_PANEL_COLS) {
        const int nrows = min(nbs - k0, (int)PG_PANEL_ROWS), kend = min((int)PG_PANEL_COLS, nbs - k0);
        __syncthreads();
        for (int i = t; i < nrows * PG_LD; i += PG_THREADS) c.panel[i] = c.AB[(size_t)k0 * PG_LD + i];
        __syncthreads();
        for (int kk = 0; kk < kend; kk++) {
            const double piv = c.panel[kk * PG_LD];
            if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }      // (the same value in every thread: uniform)
            const double inv = 1.0 / sqrt(piv);
            if (t >= 1 && t <= PG_BW && k0 + kk + t < nbs) c.panel[(kk + t) * PG_LD + t] *= inv;      // column kk of the factor, in place
            if (t == 0) c.dinv_band[kk] = inv;
            __syncthreads();
            if (d1 > 0 && k0 + kk + d1 < nbs) c.panel[(kk + d1) * PG_LD + (d1 - d2)] -= c.panel[(kk + d1) * PG_LD + d1] * c.panel[(kk + d2) * PG_LD + d2];
            __syncthreads();
        }
        // the panel goes back as a whole: finished rows of the factor (1 / L_kk on the diagonal) and the partly updated rows behind them
        if (ok) for (int i = t; i < nrows * PG_LD; i += PG_THREADS) c.AB[(size_t)k0 * PG_LD + i] = (i % PG_LD == 0 && i / PG_LD < kend) ? c.dinv_band[i / PG_LD] : c.panel[i];
    }
    __syncthreads();
    if (!ok) return false;
    // 2. border rows and the right-hand side (row m) through the band factor: W <- W L^-T, the last PG_BW values in registers.  A chunk
    // of PG_LD columns loads first and stores last: no store sits between the loads, so they are all in flight together
    for (int r = t; r < M1; r += PG_THREADS) {
        double w[PG_LD], in[PG_LD];
#pragma unroll
        for (int i = 0; i < PG_LD; i++) w[i] = 0.0;
        for (int k0 = 0; k0 < nbs; k0 += PG_LD) {
#pragma unroll
            for (int kk = 0; kk < PG_LD; kk++) in[kk] = k0 + kk < nbs ? c.W[(size_t)(k0 + kk) * M1 + r] : 0.0;
#pragma unroll
            for (int kk = 0; kk < PG_LD; kk++) {
                const double *Lr = c.AB + (size_t)(k0 + kk) * PG_LD;      // (rows past the end are zero padding)
                double acc = in[kk];
#pragma unroll
                for (int d = 1; d <= PG_BW; d++) acc -= w[(kk - d + PG_LD) % PG_LD] * Lr[d];      // (Lr[d] is 0 where k - d < 0)
                w[kk] = acc * Lr[0];
            }
#pragma unroll
            for (int kk = 0; kk < PG_LD; kk++) if (k0 + kk < nbs) c.W[(size_t)(k0 + kk) * M1 + r] = w[kk];
        }
    }
    __syncthreads();
    // 3. Schur complement S -= W W^T (rows 0 .. m, columns 0 .. m-1, lower triangle), 4 x 4 per thread, k ascending
    {
        const int ty = t / 16, tx = t % 16, wave = t / 64, lane = t % 64;
        // a 64 x 64 tile of S per pass; W goes through LDS in chunks of PG_KC columns (rows of the tile | columns of the tile), loaded
        // coalesced with every load of a chunk in flight at once
        double *At = c.panel, *Bt = c.panel + PG_KC * 64;
        for (int R0 = 0; R0 < M1; R0 += 64)
            for (int C0 = 0; C0 <= R0 && C0 < m; C0 += 64) {
                const int r0 = R0 + 4 * ty, c0 = C0 + 4 * tx;
                double acc[16];
                for (int i = 0; i < 16; i++) acc[i] = 0.0;
                for (int k0 = 0; k0 < nbs; k0 += PG_KC) {
                    const int kn = min((int)PG_KC, nbs - k0);
                    __syncthreads();
                    for (int i = t; i < 2 * PG_KC * 64; i += PG_THREADS) {
                        const int half = i / (PG_KC * 64), kk = (i / 64) % PG_KC, col = i % 64;
                        const int row = min((half ? C0 : R0) + col, M1 - 1);      // (past the matrix: a copy of the last row, never written back)
                        c.panel[i] = kk < kn ? c.W[(size_t)(k0 + kk) * M1 + row] : 0.0;
                    }
                    __syncthreads();
                    for (int kk = 0; kk < kn; kk++) {
                        double a[4], bq[4];
                        for (int i = 0; i < 4; i++) { a[i] = At[kk * 64 + 4 * ty + i]; bq[i] = Bt[kk * 64 + 4 * tx + i]; }
                        for (int i = 0; i < 4; i++)
                            for (int j = 0; j < 4; j++) acc[4 * i + j] += a[i] * bq[j];
                    }
                }
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++) {
                        const int r = r0 + i, cc = c0 + j;
                        if (r < M1 && cc < m && cc <= r) c.S[(size_t)r * M1 + cc] -= acc[4 * i + j];
                    }
            }
        __syncthreads();
        // dense Cholesky of the border; column k of the factor goes to row k of the unused upper triangle, the right-hand side rides as row m
        for (int k = 0; k < m; k++) {
            const double piv = c.S[(size_t)k * M1 + k];
            if (!(piv > 0.0) || !(piv < 1e300)) { ok = false; break; }
            const double inv = 1.0 / sqrt(piv);
            for (int r = k + 1 + t; r <= m; r += PG_THREADS) {      // column k of the factor: to LDS for the update, to row k for the back substitution
                const double l = c.S[(size_t)r * M1 + k] * inv;
                c.panel[r] = l;
                c.S[(size_t)k * M1 + r] = l;
            }
            if (t == 0) c.dinv[k] = inv;
            __syncthreads();
            for (int r = k + 1 + wave; r <= m; r += 16) {      // a wave takes rows r, r + 4, r + 8, r + 12, its lanes along them: four loads in flight
                double lr[4];
                int ce[4], cmax = -1;
                for (int i = 0; i < 4; i++) {
                    const int rr = r + 4 * i;
                    lr[i] = rr <= m ? c.panel[rr] : 0.0;
                    ce[i] = rr <= m ? min(rr, m - 1) : -1;
                    cmax = max(cmax, ce[i]);
                }
                for (int cc = k + 1 + lane; cc <= cmax; cc += 64) {
                    const double lc = c.panel[cc];
                    double v[4];
                    for (int i = 0; i < 4; i++) v[i] = cc <= ce[i] ? c.S[(size_t)(r + 4 * i) * M1 + cc] : 0.0;
                    for (int i = 0; i < 4; i++) if (cc <= ce[i]) c.S[(size_t)(r + 4 * i) * M1 + cc] = v[i] - lr[i] * lc;
                }
            }
            __syncthreads();
        }
        if (!ok) { __syncthreads(); return false; }
    }
    // 4. border back substitution L^T xs = z (z_k = S[k][m], L[r][k] = S[k][r]); z is updated in place, one column per barrier
    for (int k = m - 1; k >= 0; k--) {
        const double xk = c.S[(size_t)k * M1 + m] * c.dinv[k];
        if (t == 0) c.xs[k] = xk;
        for (int j = t; j < k; j += PG_THREADS) c.S[(size_t)j * M1 + m] -= c.S[(size_t)j * M1 + k] * xk;
        __syncthreads();
    }
    // band: L^T xb = y - W^T xs, y = row m of W
    for (int k = t; k < nbs; k += PG_THREADS) {
        const double *Wk = c.W + (size_t)k * M1;
        double acc = Wk[m];
        for (int r = 0; r < m; r++) acc -= Wk[r] * c.xs[r];
        c.tvec[k] = acc;
    }
    __syncthreads();
    if (t == 0) {      // serial: each unknown needs the PG_BW behind it (kept in registers); loads first, stores last, as above
        double w[PG_LD], in[PG_LD];
#pragma unroll
        for (int i = 0; i < PG_LD; i++) w[i] = 0.0;
        for (int j0 = 0; j0 < nbs; j0 += PG_LD) {
#pragma unroll
            for (int jj = 0; jj < PG_LD; jj++) in[jj] = j0 + jj < nbs ? c.tvec[nbs - 1 - (j0 + jj)] : 0.0;
#pragma unroll
            for (int jj = 0; jj < PG_LD; jj++) {
                const int k = max(nbs - 1 - (j0 + jj), 0);      // (past the first unknown: a value nobody reads)
                double acc = in[jj];
#pragma unroll
                for (int d = 1; d <= PG_BW; d++) acc -= c.AB[(size_t)(k + d) * PG_LD + d] * w[(jj - d + PG_LD) % PG_LD];      // (rows past the end are zero padding)
                w[jj] = acc * c.AB[(size_t)k * PG_LD];
            }
#pragma unroll
            for (int jj = 0; jj < PG_LD; jj++) if (j0 + jj < nbs) c.tvec[nbs - 1 - (j0 + jj)] = w[jj];
        }
    }
    __syncthreads();
    double bad = 0.0;
    for (int k = t; k < nbs + m; k += PG_THREADS) {
        const double y = k < nbs ? c.tvec[k] : c.xs[k - nbs];
        const double d = -c.scale[k] * y;
        c.delta[k] = d;
        if (!(fabs(d) < 1e300)) bad = 1.0;
    }
    return pg_block_max(bad, c.red) == 0.0;
}

__global__ void __launch_bounds__(PG_THREADS) pose_graph_kernel(int n_graphs, const PgHdr *hdrs, const int *ipool, const double *dpool, double *scratch,
                                                                double *out, PgOpts opts) {
    __shared__ double s_red[PG_THREADS];
    __shared__ double s_panel[PG_PANEL_ROWS * PG_LD];
    __shared__ double s_dinv[PG_PANEL_ROWS];
    const int gidx = blockIdx.x, t = threadIdx.x;
    if (gidx >= n_graphs) return;
    const PgHdr H = hdrs[gidx];
    const PgScratch L(H.n_nodes, H.n_free, H.nb, H.nk, H.n_edges);
    PgCtx c;
    c.N = H.n_nodes; c.F = H.n_free; c.nb = H.nb; c.nk = H.nk; c.E = H.n_edges; c.nbs = 4 * H.nb; c.m = 4 * H.nk; c.M1 = c.m + 1;
    const int *ip = ipool + H.o_int;
    c.pos = ip; c.ea = c.pos + c.N; c.eb = c.ea + c.E; c.ek = c.eb + c.E; c.nodeof = c.ek + c.E; c.cptr = c.nodeof + c.F; c.cent = c.cptr + c.F + 1;
    double *s = scratch + H.o_scr;
    c.ypr = s + L.ypr; c.x = s + L.x; c.xc = s + L.xc; c.meas = s + L.meas; c.scale = s + L.scale; c.delta = s + L.delta; c.dinv = s + L.dinv;
    c.xs = s + L.xs; c.tvec = s + L.tvec; c.AB = s + L.AB; c.W = s + L.W; c.S = s + L.S;
    c.o = opts; c.red = s_red; c.panel = s_panel; c.dinv_band = s_dinv;
    const double *tin = dpool + H.o_dbl, *qin = tin + 3 * c.N, *lmeas = qin + 4 * c.N;
    double *o_t = out + H.o_out, *o_R = o_t + 3 * c.N, *o_sum = o_R + 9 * c.N;

    // ---- Euler angles and initial values (:456-466), the factor storage's zero padding
    for (int i = t; i < c.N; i += PG_THREADS) {
        double e[3];
        r2ypr(to_matrix(Quat(qin + 4 * i)), e);
        for (int k = 0; k < 3; k++) c.ypr[3 * i + k] = e[k];
        c.x[4 * i] = e[0];
        for (int k = 0; k < 3; k++) c.x[4 * i + 1 + k] = tin[3 * i + k];
    }
    for (int i = t; i < PG_LD * PG_LD; i += PG_THREADS) c.AB[(size_t)PG_LD * c.nbs + i] = 0.0;
    for (int i = t; i < PG_SUM; i += PG_THREADS) o_sum[i] = 0.0;
    __syncthreads();
    // ---- measurements: sequence edges from the input poses (:484-489), loop edges from the caller with the older node's pitch and roll
    for (int e = t; e < c.E; e += PG_THREADS) {
        const int a = c.ea[e], b = c.eb[e], kd = c.ek[e];
        double *me = c.meas + 6 * e;
        if (kd == 0) {
            const V3 rel = rotate(inverse(Quat(qin + 4 * a)), V3(tin[3 * b] - tin[3 * a], tin[3 * b + 1] - tin[3 * a + 1], tin[3 * b + 2] - tin[3 * a + 2]));
            me[0] = rel.x; me[1] = rel.y; me[2] = rel.z; me[3] = c.ypr[3 * b] - c.ypr[3 * a];
        } else {
            for (int k = 0; k < 4; k++) me[k] = lmeas[4 * (kd - 1) + k];
        }
        me[4] = c.ypr[3 * a + 1]; me[5] = c.ypr[3 * a + 2];
    }
    __syncthreads();
    // the (d1, d2) pair of the band update this thread owns: 1 <= d2 <= d1 <= PG_BW, 190 pairs
    int d1 = 0, d2 = 0;
    {
        int q = t;
        for (int a = 1; a <= PG_BW; a++) { if (q < a) { d1 = a; d2 = q + 1; break; } q -= a; }
    }

    // ---- TrustRegionMinimizer with LevenbergMarquardtStrategy
    double fixed_cost = 0.0;
    double cost = pg_cost(c, c.x, &fixed_cost);
    const double initial_cost = cost;
    int n_rec = 0, termination = 0;
    auto record = [&](double cst, double cand, double rho, double radius, int step) {
        if (t == 0 && n_rec < PG_T) {
            o_sum[15 + n_rec] = cst; o_sum[15 + PG_T + n_rec] = cand; o_sum[15 + 2 * PG_T + n_rec] = rho; o_sum[15 + 3 * PG_T + n_rec] = radius;
            o_sum[15 + 4 * PG_T + 2 + n_rec] = (double)step;
        }
        n_rec++;
    };
    record(cost, 0.0, 0.0, opts.radius0, 1);
    bool done = false;
    if (c.F == 0) { termination = 1; done = true; }      // nothing free: the gradient is empty
    if (!done) {
        pg_node_pass(c, 0);
        __syncthreads();
        if (pg_node_pass(c, 1) <= opts.gtol) { termination = 1; done = true; }
    }
    double radius = opts.radius0, decrease_factor = 2.0;
    int invalid = 0, iter = 0;
    while (!done) {
        if (iter >= opts.max_it) { termination = 0; break; }
        if (radius < 1e-32) { termination = 4; break; }
        iter++;
        pg_assemble(c, radius);
        bool valid = pg_solve(c, d1, d2);
        double mcc = 0.0;
        if (valid) { mcc = pg_model_cost_change(c); valid = mcc > 0.0; }
        if (!valid) {
            record(cost, 0.0, 0.0, radius, -1);
            if (++invalid >= PG_MAX_INVALID) { termination = 5; break; }
            radius *= 0.5;      // LevenbergMarquardtStrategy::StepIsInvalid
            continue;
        }
        invalid = 0;
        // candidate: Plus with the angle wrapped (pose_graph.h:99-115); constant nodes keep their values
        double dx2 = 0.0, x2 = 0.0;
        for (int i = t; i < c.N; i += PG_THREADS) {
            const int p = c.pos[i];
            for (int k = 0; k < 4; k++) {
                const double xv = c.x[4 * i + k];
                double v = xv;
                if (p >= 0) {
                    v = xv + c.delta[4 * p + k];
                    if (k == 0) v = pg_normalize_angle(v);
                    dx2 += (v - xv) * (v - xv); x2 += xv * xv;
                }
                c.xc[4 * i + k] = v;
            }
        }
        dx2 = pg_block_sum(dx2, c.red); x2 = pg_block_sum(x2, c.red);
        const double cand = pg_cost(c, c.xc, nullptr);
        const double cost_change = cost - cand, rho = cost_change / mcc;
        if (sqrt(dx2) <= opts.ptol * (sqrt(x2) + opts.ptol)) { record(cost, cand, rho, radius, 0); termination = 2; break; }
        if (fabs(cost_change) <= opts.ftol * cost) { record(cost, cand, rho, radius, 0); termination = 3; break; }
        if (rho > opts.min_rel_dec) {
            for (int i = t; i < 4 * c.N; i += PG_THREADS) c.x[i] = c.xc[i];
            __syncthreads();
            cost = cand;
            record(cost, cand, rho, radius, 1);
            const double q = 2.0 * rho - 1.0;      // LevenbergMarquardtStrategy::StepAccepted
            radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
            decrease_factor = 2.0;
            if (pg_node_pass(c, 1) <= opts.gtol) { termination = 1; break; }
        } else {
            record(cost, cand, rho, radius, 0);
            radius /= decrease_factor;      // StepRejected
            decrease_factor *= 2.0;
        }
    }
    __syncthreads();
    // ---- poses (:532-543) and drift (:549-557).  After FAILURE x still holds the last accepted state: never a NaN
    for (int i = t; i < c.N; i += PG_THREADS) {
        for (int k = 0; k < 3; k++) o_t[3 * i + k] = c.x[4 * i + 1 + k];
        const M3 R = ypr2R(c.x[4 * i], c.ypr[3 * i + 1], c.ypr[3 * i + 2]);
        for (int k = 0; k < 9; k++) o_R[9 * i + k] = R.m[k];
    }
    if (t == 0) {
        const int i = c.N - 1;
        double e[3];
        r2ypr(ypr2R(c.x[4 * i], c.ypr[3 * i + 1], c.ypr[3 * i + 2]), e);
        const double yaw_drift = e[0] - c.ypr[3 * i];
        const M3 Rd = ypr2R(yaw_drift, 0.0, 0.0);
        const V3 td = V3(c.x + 4 * i + 1) - Rd * V3(tin + 3 * i);
        o_sum[0] = initial_cost + fixed_cost; o_sum[1] = cost + fixed_cost; o_sum[2] = yaw_drift;
        for (int k = 0; k < 9; k++) o_sum[3 + k] = Rd.m[k];
        o_sum[12] = td.x; o_sum[13] = td.y; o_sum[14] = td.z;
        o_sum[15 + 4 * PG_T] = (double)n_rec; o_sum[15 + 4 * PG_T + 1] = (double)termination;
    }
}

// n independent edges: in = [xi 4 | xj 4 | meas 6] per edge, out = [r 4 | Ji 16 | Jj 16 | cost]
enum { PG_EDGE_IN = 14, PG_EDGE_OUT = 37 };
__global__ void __launch_bounds__(64) pose_graph_edges_kernel(int n, const int *kind, const double *in, double *out, PgOpts opts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *e = in + (size_t)PG_EDGE_IN * i;
    double r[4], Ji[16], Jj[16];
    const double cost = pg_edge(kind[i] != 0, e, e + 4, e + 8, opts, true, r, Ji, Jj);
    double *o = out + (size_t)PG_EDGE_OUT * i;
    for (int k = 0; k < 4; k++) o[k] = r[k];
    for (int k = 0; k < 16; k++) { o[4 + k] = Ji[k]; o[20 + k] = Jj[k]; }
    o[36] = cost;
}

}  // namespace tcv
using namespace tcv;

// ---------------------------------------------------------------------------------------------------------------- host side
namespace {

struct PgPlan {
    int N = 0, F = 0, nb = 0, nk = 0, E = 0, E_fixed = 0;
    std::vector<int> ints;      // pos N | ea E | eb E | ek E | nodeof F | cptr F + 1 | cent
};

int pg_validate(const tcv_pose_graph_desc &d, int g) {
    const std::string at = "pose graph " + std::to_string(g) + ": ";
    if (d.n_nodes < 1) { set_error(at + "n_nodes < 1"); return TCV_ERR_INVALID; }
    if (!d.t || !d.q_xyzw) { set_error(at + "missing array (t, q_xyzw)"); return TCV_ERR_INVALID; }
    if (d.n_loops < 0) { set_error(at + "n_loops < 0"); return TCV_ERR_INVALID; }
    if (d.n_loops > 0 && (!d.loop_cur || !d.loop_old || !d.loop_relative_t || !d.loop_relative_yaw)) { set_error(at + "missing array (loop edges)"); return TCV_ERR_INVALID; }
    for (int l = 0; l < d.n_loops; l++) {
        if (d.loop_cur[l] < 0 || d.loop_cur[l] >= d.n_nodes || d.loop_old[l] < 0 || d.loop_old[l] >= d.n_nodes) { set_error(at + "loop index out of range"); return TCV_ERR_INVALID; }
        if (d.loop_old[l] >= d.loop_cur[l]) { set_error(at + "loop_old >= loop_cur"); return TCV_ERR_INVALID; }
    }
    bool fin = true;
    // (after the limits would be cheaper, but the contract is: invalid input is reported as invalid)
    for (long long i = 0; i < 3LL * d.n_nodes; i++) fin = fin && std::isfinite(d.t[i]);
    for (long long i = 0; i < 4LL * d.n_nodes; i++) fin = fin && std::isfinite(d.q_xyzw[i]);
    for (long long i = 0; i < 3LL * d.n_loops; i++) fin = fin && std::isfinite(d.loop_relative_t[i]);
    for (int i = 0; i < d.n_loops; i++) fin = fin && std::isfinite(d.loop_relative_yaw[i]);
    if (!fin) { set_error(at + "non-finite input"); return TCV_ERR_INVALID; }
    for (int i = 0; i < d.n_nodes; i++) {
        const double *q = d.q_xyzw + 4 * i;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) { set_error(at + "zero quaternion"); return TCV_ERR_INVALID; }
    }
    if (d.n_nodes > TCV_POSE_GRAPH_MAX_NODES || d.n_loops > TCV_POSE_GRAPH_MAX_LOOPS) {
        set_error(at + "beyond TCV_POSE_GRAPH_MAX_NODES / TCV_POSE_GRAPH_MAX_LOOPS"); return TCV_ERR_UNSUPPORTED;
    }
    return TCV_OK;
}

// graph construction of :445-519 and the elimination order
int pg_plan(const tcv_pose_graph_desc &d, PgPlan &P) {
    const int N = d.n_nodes;
    auto seq = [&](int i) { return d.sequence ? d.sequence[i] : 1; };
    std::vector<char> is_const(N), border(N, 0);
    for (int i = 0; i < N; i++) is_const[i] = i == 0 || seq(i) == 0;
    std::vector<int> ea, eb, ek;
    std::vector<std::vector<int>> loops_at(N);
    for (int l = 0; l < d.n_loops; l++) loops_at[d.loop_cur[l]].push_back(l);
    for (int i = 0; i < N; i++) {
        for (int j = 1; j < 5; j++)
            if (i - j >= 0 && seq(i) == seq(i - j)) { ea.push_back(i - j); eb.push_back(i); ek.push_back(0); }
        for (int l : loops_at[i]) {
            ea.push_back(d.loop_old[l]); eb.push_back(i); ek.push_back(1 + l);
            if (!is_const[i] && !is_const[d.loop_old[l]]) border[i] = 1;
        }
    }
    const int E = (int)ea.size();
    std::vector<int> pos(N, -1), nodeof;
    for (int i = 0; i < N; i++) if (!is_const[i] && !border[i]) { pos[i] = (int)nodeof.size(); nodeof.push_back(i); }
    const int nb = (int)nodeof.size();
    for (int i = 0; i < N; i++) if (!is_const[i] && border[i]) { pos[i] = (int)nodeof.size(); nodeof.push_back(i); }
    const int F = (int)nodeof.size();
    std::vector<std::vector<int>> inc(F);
    int fixed = 0;
    for (int e = 0; e < E; e++) {
        const int pa = pos[ea[e]], pb = pos[eb[e]];
        if (pa < 0 && pb < 0) fixed++;
        if (pa >= 0) inc[pa].push_back(2 * e);
        if (pb >= 0) inc[pb].push_back(2 * e + 1);
        if (pa >= 0 && pb >= 0 && pa < nb && pb < nb && std::abs(pa - pb) > 4) { set_error("pose graph: band wider than four nodes"); return TCV_ERR_UNSUPPORTED; }
    }
    P.N = N; P.F = F; P.nb = nb; P.nk = F - nb; P.E = E; P.E_fixed = fixed;
    P.ints.clear();
    P.ints.insert(P.ints.end(), pos.begin(), pos.end());
    P.ints.insert(P.ints.end(), ea.begin(), ea.end());
    P.ints.insert(P.ints.end(), eb.begin(), eb.end());
    P.ints.insert(P.ints.end(), ek.begin(), ek.end());
    P.ints.insert(P.ints.end(), nodeof.begin(), nodeof.end());
    int run = 0;
    for (int p = 0; p < F; p++) { P.ints.push_back(run); run += (int)inc[p].size(); }
    P.ints.push_back(run);
    for (int p = 0; p < F; p++) P.ints.insert(P.ints.end(), inc[p].begin(), inc[p].end());
    return TCV_OK;
}

PgOpts pg_opts(const tcv_pose_graph_options *o) {
    tcv_pose_graph_options d;
    tcv_pose_graph_options_default(&d);
    if (o) d = *o;
    PgOpts r;
    r.max_it = d.max_num_iterations; r.pad_ = 0; r.huber = d.huber_delta; r.weight = d.loop_weight; r.yaw_div = d.loop_yaw_divisor;
    r.ftol = d.function_tolerance; r.gtol = d.gradient_tolerance; r.ptol = d.parameter_tolerance; r.radius0 = d.initial_trust_region_radius;
    r.min_rel_dec = d.min_relative_decrease;
    return r;
}
int pg_check_opts(const tcv_pose_graph_options *o) {
    if (!o) return TCV_OK;
    const double v[] = {o->huber_delta, o->loop_weight, o->loop_yaw_divisor, o->function_tolerance, o->gradient_tolerance, o->parameter_tolerance,
                        o->initial_trust_region_radius, o->min_relative_decrease};
    for (double x : v) if (!std::isfinite(x)) { set_error("pose graph: non-finite option"); return TCV_ERR_INVALID; }
    if (o->max_num_iterations < 0 || !(o->loop_yaw_divisor != 0.0) || !(o->initial_trust_region_radius > 0.0)) { set_error("pose graph: bad option"); return TCV_ERR_INVALID; }
    return TCV_OK;
}

thread_local double g_pg_timing[4] = {0, 0, 0, 0};      // host packing, upload, kernel, download of the calling thread's last batch, ms

}  // namespace

extern "C" void tcv_pose_graph_options_default(tcv_pose_graph_options *o) {
    if (!o) return;
    o->max_num_iterations = 5; o->huber_delta = 0.1; o->loop_weight = 1.0; o->loop_yaw_divisor = 10.0;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->initial_trust_region_radius = 1e4; o->min_relative_decrease = 1e-3;
}

extern "C" int tcv_pose_graph_plan_stats(const tcv_pose_graph_desc *desc, long long *out, int *position) {
    if (!desc || !out) { set_error("pose_graph_plan_stats: bad argument"); return TCV_ERR_INVALID; }
    if (int rc = pg_validate(*desc, 0)) return rc;
    PgPlan P;
    if (int rc = pg_plan(*desc, P)) return rc;
    const PgScratch L(P.N, P.F, P.nb, P.nk, P.E);
    out[0] = P.F; out[1] = P.nb; out[2] = P.nk; out[3] = P.E - P.E_fixed; out[4] = P.E_fixed; out[5] = PG_BW; out[6] = 8 * L.total; out[7] = 0;
    if (position) std::memcpy(position, P.ints.data(), sizeof(int) * P.N);
    return TCV_OK;
}

// the calling thread's last tcv_pose_graphs_optimize: out[4] = host packing, upload, kernel, download in ms (device times from events)
extern "C" int tcv_pose_graph_last_timing(double *out) {
    if (!out) { set_error("pose_graph_last_timing: bad argument"); return TCV_ERR_INVALID; }
    for (int k = 0; k < 4; k++) out[k] = g_pg_timing[k];
    return TCV_OK;
}

extern "C" int tcv_pose_graphs_optimize(int n, const tcv_pose_graph_desc *descs, const tcv_pose_graph_options *options, double *const *t_out,
                                        double *const *R_out, tcv_pose_graph_summary *summaries, void *hip_stream) {
    if (n < 1 || !descs || !summaries) { set_error("pose_graphs_optimize: bad argument"); return TCV_ERR_INVALID; }
    if (int rc = pg_check_opts(options)) return rc;
    int worst = TCV_OK;
    for (int g = 0; g < n; g++) {      // every graph is validated before a limit is reported
        const int rc = pg_validate(descs[g], g);
        if (rc == TCV_ERR_INVALID) return rc;
        if (rc) worst = rc;
    }
    if (worst) return worst;
    if (n > TCV_POSE_GRAPH_MAX_BATCH) { set_error("pose_graphs_optimize: beyond TCV_POSE_GRAPH_MAX_BATCH"); return TCV_ERR_UNSUPPORTED; }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<PgPlan> plans(n);
    std::vector<PgHdr> hdrs(n);
    long long n_int = 0, n_dbl = 0, n_scr = 0, n_out = 0;
    for (int g = 0; g < n; g++) {
        if (int rc = pg_plan(descs[g], plans[g])) return rc;
        const PgPlan &P = plans[g];
        PgHdr &H = hdrs[g];
        H.n_nodes = P.N; H.n_free = P.F; H.nb = P.nb; H.nk = P.nk; H.n_edges = P.E; H.n_loops = descs[g].n_loops; H.pad0_ = H.pad1_ = 0;
        H.o_int = n_int; H.o_dbl = n_dbl; H.o_scr = n_scr; H.o_out = n_out;
        n_int += (long long)P.ints.size();
        n_dbl += 7LL * P.N + 4LL * descs[g].n_loops;
        n_scr += PgScratch(P.N, P.F, P.nb, P.nk, P.E).total;
        n_out += 12LL * P.N + PG_SUM;
    }
    if (int rc = device_ready()) return rc;
    // one upload: [headers | input doubles | ints], one device allocation: [upload | output | scratch]
    const size_t b_hdr = sizeof(PgHdr) * (size_t)n, b_dbl = 8 * (size_t)n_dbl, b_int = ((4 * (size_t)n_int + 7) / 8) * 8;
    const size_t b_in = b_hdr + b_dbl + b_int, b_out = 8 * (size_t)n_out, b_scr = 8 * (size_t)n_scr;
    hipStream_t st = tcv::resolve_stream(hip_stream);
    tcv::StagedTransfer tr(st, b_in + b_out);
    if (!tr.host) { set_error("hipHostMalloc (pose graph staging) failed"); return TCV_ERR_HIP; }
    char *h = (char *)tr.host;
    std::memcpy(h, hdrs.data(), b_hdr);
    double *hd = (double *)(h + b_hdr);
    int *hi = (int *)(h + b_hdr + b_dbl);
    for (int g = 0; g < n; g++) {
        const tcv_pose_graph_desc &d = descs[g];
        double *p = hd + hdrs[g].o_dbl;
        std::memcpy(p, d.t, 24 * (size_t)d.n_nodes); p += 3 * d.n_nodes;
        std::memcpy(p, d.q_xyzw, 32 * (size_t)d.n_nodes); p += 4 * d.n_nodes;
        for (int l = 0; l < d.n_loops; l++) { p[4 * l] = d.loop_relative_t[3 * l]; p[4 * l + 1] = d.loop_relative_t[3 * l + 1]; p[4 * l + 2] = d.loop_relative_t[3 * l + 2]; p[4 * l + 3] = d.loop_relative_yaw[l]; }
        std::memcpy(hi + hdrs[g].o_int, plans[g].ints.data(), sizeof(int) * plans[g].ints.size());
    }
    const auto t1 = std::chrono::steady_clock::now();
    hipError_t e = tr.dev_alloc(b_in + b_out + b_scr);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (pose graph batch)");
    char *dv = (char *)tr.dev;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = true;
    for (int k = 0; k < 4; k++) timed = timed && hipEventCreate(&ev[k]) == hipSuccess;
    tr.issued();
    if (timed) (void)hipEventRecord(ev[0], st);
    e = hipMemcpyAsync(dv, h, b_in, hipMemcpyHostToDevice, st);
    if (timed) (void)hipEventRecord(ev[1], st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pose_graph_kernel, dim3(n), dim3(PG_THREADS), 0, st, n, (const PgHdr *)dv, (const int *)(dv + b_hdr + b_dbl),
                           (const double *)(dv + b_hdr), (double *)(dv + b_in + b_out), (double *)(dv + b_in), pg_opts(options));
        e = hipGetLastError();
    }
    if (timed) (void)hipEventRecord(ev[2], st);
    if (e == hipSuccess) e = hipMemcpyAsync(h + b_in, dv + b_in, b_out, hipMemcpyDeviceToHost, st);
    if (timed) (void)hipEventRecord(ev[3], st);
    if (e == hipSuccess) e = tr.wait();
    g_pg_timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    for (int k = 0; k < 3; k++) {
        float ms = 0.0f;
        if (timed && e == hipSuccess && hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_pg_timing[1 + k] = ms; else g_pg_timing[1 + k] = 0.0;
    }
    for (int k = 0; k < 4; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (e != hipSuccess) return hip_fail(e, "pose_graphs_optimize");
    const double *ho = (const double *)(h + b_in);
    for (int g = 0; g < n; g++) {
        const PgPlan &P = plans[g];
        const double *o = ho + hdrs[g].o_out, *s = o + 12LL * P.N;
        if (t_out && t_out[g]) std::memcpy(t_out[g], o, 24 * (size_t)P.N);
        if (R_out && R_out[g]) std::memcpy(R_out[g], o + 3LL * P.N, 72 * (size_t)P.N);
        tcv_pose_graph_summary &S = summaries[g];
        std::memset(&S, 0, sizeof S);
        S.iterations = (int)s[15 + 4 * PG_T]; S.termination = (int)s[15 + 4 * PG_T + 1];
        S.num_free_nodes = P.F; S.num_edges = P.E - P.E_fixed;
        S.initial_cost = s[0]; S.final_cost = s[1]; S.yaw_drift = s[2];
        std::memcpy(S.r_drift, s + 3, 72); std::memcpy(S.t_drift, s + 12, 24);
        for (int k = 0; k < PG_T; k++) {
            S.cost[k] = s[15 + k]; S.cost_candidate[k] = s[15 + PG_T + k]; S.rho[k] = s[15 + 2 * PG_T + k]; S.radius[k] = s[15 + 3 * PG_T + k];
            S.step[k] = (int)s[15 + 4 * PG_T + 2 + k];
        }
    }
    return TCV_OK;
}

extern "C" int tcv_pose_graph_eval_edges(int n, const int *kind, const double *yaw_i, const double *t_i, const double *yaw_j, const double *t_j,
                                         const double *measurement, const tcv_pose_graph_options *options, double *residual, double *jacobian, double *cost) {
    if (n < 1 || n > (1 << 20) || !kind || !yaw_i || !t_i || !yaw_j || !t_j || !measurement || !residual || !jacobian || !cost) { set_error("pose_graph_eval_edges: bad argument"); return TCV_ERR_INVALID; }
    if (int rc = pg_check_opts(options)) return rc;
    std::vector<double> in((size_t)PG_EDGE_IN * n);
    for (int i = 0; i < n; i++) {
        double *c = in.data() + (size_t)PG_EDGE_IN * i;
        c[0] = yaw_i[i]; std::memcpy(c + 1, t_i + 3 * i, 24); c[4] = yaw_j[i]; std::memcpy(c + 5, t_j + 3 * i, 24); std::memcpy(c + 8, measurement + 6 * i, 48);
        if (kind[i] != 0 && kind[i] != 1) { set_error("pose_graph_eval_edges: kind is 0 or 1"); return TCV_ERR_INVALID; }
    }
    for (double v : in) if (!std::isfinite(v)) { set_error("pose_graph_eval_edges: non-finite input"); return TCV_ERR_INVALID; }
    if (int rc = device_ready()) return rc;
    const size_t b_in = 8 * in.size(), b_out = 8 * (size_t)PG_EDGE_OUT * n;
    tcv::RoundTrip rt(tcv::util_stream(), b_in + 4 * (size_t)n, b_out);      // [edges | kind (ints)] -> n records of PG_EDGE_OUT doubles
    if (int rc = rt.ready("pose_graph_eval_edges")) return rc;
    std::memcpy(rt.h_in<char>(), in.data(), b_in);
    std::memcpy(rt.h_in<char>() + b_in, kind, 4 * (size_t)n);
    if (int rc = rt.run("pose_graph_eval_edges", [&](hipStream_t st) {
            hipLaunchKernelGGL(pose_graph_edges_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, (const int *)(rt.d_in<char>() + b_in), (const double *)rt.d_in(), rt.d_out(), pg_opts(options));
        })) return rc;
    const double *o = rt.h_out();
    for (int i = 0; i < n; i++) {
        std::memcpy(residual + 4 * i, o + (size_t)PG_EDGE_OUT * i, 32);
        std::memcpy(jacobian + 32 * i, o + (size_t)PG_EDGE_OUT * i + 4, 256);
        cost[i] = o[(size_t)PG_EDGE_OUT * i + 36];
    }
    return TCV_OK;
}
