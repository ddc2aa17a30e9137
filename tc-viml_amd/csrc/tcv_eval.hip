// tcv::evaluate_kernel -- ceres::Problem::Evaluate(options, &cost, &residuals, &gradient, nullptr) for every window of a resident batch:
// the robustified cost by factor family, the residual vector, one cost per residual block and the tangent-space gradient J'r at either
// the uploaded initial states or the states the last solve left.  It reads the batch as the solve kernel does (tcv_packed.h) and uses
// the same factor code (tcv_factors.h); nothing of the solve / marginalisation kernels is touched.
//
// One 256-thread workgroup per window, states in LDS, a few KB of LDS otherwise (several workgroups per CU).  Every sum has a fixed
// order that depends on the window alone -- never on the batch, the grid or the timing: family costs are per-thread partial sums (factor
// f on thread f mod 256, ascending) folded by a fixed tree; a gradient entry is added by its OWNER thread from the J'r pieces the factors
// left in the window's staging area, in factor order (owner lists: tcv_eval.h; built by the host once per plan, tcv_eval_host.cpp); the
// max-norm is a maximum.  No atomics.
#include <hip/hip_runtime.h>

#include "tcv_dev.h"
#include "tcv_eval.h"
#include "tcv_factors.h"

namespace tcv {

// sum over the workgroup in a fixed tree (thread t holds v; the result is returned to every thread)
__device__ __forceinline__ double ev_block_sum(double v, lds_d *red, int tid) {
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}
// maximum that keeps a NaN (the host reports TCV_ERR_NUMERIC on one)
__device__ __forceinline__ double ev_max_nan(double a, double b) { return (a != a || a > b) ? a : b; }

__global__ void __launch_bounds__(256) evaluate_kernel(EvalArgs A) {
    extern __shared__ __attribute__((aligned(16))) double ev_lds_raw[];
    const int tid = threadIdx.x;
    const int win = blockIdx.x;
    if (win >= A.nwin) return;
    lds_d *lds = (lds_d *)ev_lds_raw;
    lds_d *x = lds, *red = x + A.state_stride, *pdx = red + 256, *pr = pdx + 128, *ws = pr + 128;

    cst_win *W = (cst_win *)(A.win + win);
    cst_plan &P = *(cst_plan *)(A.plans + W->plan);
    cst_i *ip = (cst_i *)(A.ipool + A.plan_base[W->plan]);
    cst_d *dp = (cst_d *)(A.dpool + W->dbase);
    cst_i *blk = ip + P.o_blk;
    cst_d *misc = dp + W->d_misc;
    const int nx = P.nx, L = P.nland, nc = P.nc, n_imu = P.n_imu, n_proj = P.n_proj, n_line = P.n_line, pn = P.prior_n;
    const bool want_g = A.gradient != nullptr;
    gbl_d *res = A.residuals ? (gbl_d *)(A.residuals + (size_t)win * A.res_stride) : nullptr;
    gbl_d *bc = A.block_cost ? (gbl_d *)(A.block_cost + (size_t)win * A.blk_stride) : nullptr;
    gbl_d *stage = (gbl_d *)(A.stage + (size_t)win * A.stage_stride);
    gbl_d *g_sqrt = stage, *g_rec = g_sqrt + n_imu * 225, *piece = g_rec + n_imu * IMU_REC;
    gbl_d *pc_prior = piece, *pc_imu = pc_prior + pn, *pc_proj = pc_imu + EV_PIECE_IMU * n_imu, *pc_line = pc_proj + EV_PIECE_PROJ * n_proj;

    // ---- the evaluation point
    if (A.state) { const double *s = A.state + (size_t)win * A.state_stride; for (int i = tid; i < nx + L; i += 256) x[i] = s[i]; }
    else for (int i = tid; i < nx + L; i += 256) x[i] = dp[W->d_x + i];
    __syncthreads();

    // ---- prior: r = r0 + J0 dx (MarginalizationFactor::Evaluate, marginalization_factor.cpp:335-384); the rows below prior_k0 are exact zeros
    double fam_prior = 0.0;
    if (pn > 0) {
        const int n = pn, k0 = W->prior_k0, nr = n - k0;
        cst_d *J0 = dp + W->d_prior, *r0 = J0 + nr * n, *x0 = r0 + nr;
        if (tid < n) pdx[tid] = 0.0;
        __syncthreads();
        if (tid < P.prior_nblk) {
            cst_i *pb = ip + P.o_prior + tid * 4;
            const int gs = pb[2], xo = blk[pb[0] * 4 + 1], x0o = pb[3], ls = gs == 7 ? 6 : gs;
            double xb[16], x0b[16], d[16];
            for (int i = 0; i < gs && i < 16; i++) { xb[i] = x[xo + i]; x0b[i] = x0[x0o + i]; }
            prior_block_dx(xb, x0b, gs, d);
            for (int i = 0; i < ls; i++) if (pb[1] + i < n) pdx[pb[1] + i] = d[i];
        }
        __syncthreads();
        double r = 0.0;
        if (tid < nr) {
            r = r0[tid];
            for (int j = 0; j < n; j++) r += J0[tid + nr * j] * pdx[j];
            pr[tid] = r;
        }
        __syncthreads();
        if (res && tid < k0) res[tid] = 0.0;      // the dropped leading rows are exact zeros
        if (res && tid < nr) res[k0 + tid] = r;
        fam_prior = 0.5 * ev_block_sum(r * r, red, tid);
        if (want_g && tid < n) {      // J0' r per column (the owner lists leave out the columns of constant blocks)
            double g = 0.0;
            for (int i = 0; i < nr; i++) g += J0[i + nr * tid] * pr[i];
            pc_prior[tid] = g;
        }
    }
    if (bc && tid == 0) bc[0] = fam_prior;

    // ---- IMU factors (imu_factor.h:19-181): sqrt_info (given, or LLT(cov^-1).matrixL()^T on the device), raw record, whitening
    double fam_imu = 0.0;
    if (n_imu > 0) {
        if (W->d_sqrt >= 0) {
            for (int i = tid; i < n_imu * 225; i += 256) g_sqrt[i] = dp[W->d_sqrt + i];
        } else {
            for (int f0 = 0; f0 < n_imu; f0 += EV_SQRT_ROUND) {
                const int grp = tid >> 4, f = f0 + grp;
                if (grp < EV_SQRT_ROUND && f < n_imu)
                    (void)imu_sqrt_info_group(dp + W->d_imu + f * IMU_CONST + IMU_COV, g_sqrt + f * 225, ws + grp * 450, ws + grp * 450 + 225, tid & 15);
            }
        }
        {
            const int lane = tid & 63, wave = tid >> 6;
            if (lane < n_imu) {
                cst_i *b = ip + P.o_imu + lane * 4;
                double cst[62], G3[3] = {misc[0], misc[1], misc[2]};
#pragma unroll
                for (int i = 0; i < 62; i++) cst[i] = dp[W->d_imu + lane * IMU_CONST + i];
                imu_raw_part(wave, CGEN(x + blk[b[0] * 4 + 1]), CGEN(x + blk[b[1] * 4 + 1]), CGEN(x + blk[b[2] * 4 + 1]), CGEN(x + blk[b[3] * 4 + 1]),
                             cst, G3, GEN(g_rec + lane * IMU_REC), IMU_STRIDE_J, want_g);
            }
        }
        __syncthreads();
        lds_d *rw = ws, *uw = ws + 256, *cw = ws + 512;      // whitened residuals, S' r, block costs (the workspace is free now)
        if (tid < n_imu * 15) {
            const int f = tid / 15, i = tid - 15 * f;
            const gbl_d *S = g_sqrt + f * 225 + i * 15, *rr = g_rec + f * IMU_REC + 30;
            double r = 0.0;
            for (int k = 0; k < 15; k++) r += S[k] * rr[k * IMU_STRIDE_J];
            rw[tid] = r;
            if (res) res[pn + tid] = r;
        }
        __syncthreads();
        if (tid < n_imu) {
            double s = 0.0;
            for (int i = 0; i < 15; i++) s += rw[tid * 15 + i] * rw[tid * 15 + i];
            cw[tid] = 0.5 * s;
            if (bc) bc[1 + tid] = 0.5 * s;
        }
        if (want_g && tid < n_imu * 15) {
            const int f = tid / 15, k = tid - 15 * f;
            const gbl_d *S = g_sqrt + f * 225;
            double u = 0.0;
            for (int i = 0; i < 15; i++) u += S[i * 15 + k] * rw[f * 15 + i];
            uw[tid] = u;
        }
        __syncthreads();
        for (int f = 0; f < n_imu; f++) fam_imu += cw[f];
        if (want_g)
            for (int q = tid; q < n_imu * EV_PIECE_IMU; q += 256) {
                const int f = q / EV_PIECE_IMU, c = q - EV_PIECE_IMU * f;
                const gbl_d *J = g_rec + f * IMU_REC + c;
                double g = 0.0;
                for (int i = 0; i < 15; i++) g += J[i * IMU_STRIDE_J] * uw[f * 15 + i];
                pc_imu[q] = g;
            }
    }

    // ---- point factors (projection_factor.cpp:21-124, projection_td_factor.cpp:34-140), in plan order (sorted by landmark: the host
    // hands residuals and block costs out in the caller's order)
    const double proj_sqrt = misc[3], proj_loss = A.apply_loss ? misc[4] : 0.0, line_loss = A.apply_loss ? misc[5] : 0.0;
    const bool with_td = (P.flags & 1) != 0;
    double part = 0.0;
    for (int f = tid; f < n_proj; f += 256) {
        cst_i *pf = ip + P.o_proj + f * 4;
        const lds_d *xi = x + blk[pf[0] * 4 + 1], *xj = x + blk[pf[1] * 4 + 1], *xe = x + blk[pf[2] * 4 + 1];
        const double lam = x[nx + pf[3]];
        double r[2], J[40], pts[6];
        const int pstride = with_td ? 14 : 6;
#pragma unroll
        for (int i = 0; i < 6; i++) pts[i] = dp[W->d_proj + f * pstride + i];
        int ncol = 19;
        if (with_td) {
            double aux[8];
#pragma unroll
            for (int i = 0; i < 8; i++) aux[i] = dp[W->d_proj + f * 14 + 6 + i];
            const double tdv = x[blk[P.td_cam * 4 + 1]];
            proj_td_eval(CGEN(xi), CGEN(xj), CGEN(xe), lam, tdv, pts, aux, proj_sqrt, misc[6], misc[7], r, want_g ? J : nullptr, 20);
            ncol = 20;
        } else {
            proj_eval(CGEN(xi), CGEN(xj), CGEN(xe), lam, pts, proj_sqrt, r, want_g ? J : nullptr, 20);
        }
        const double c = loss_correct2(r, want_g ? J : nullptr, ncol, 20, proj_loss);
        part += c;
        if (res) { res[pn + 15 * n_imu + 2 * f] = r[0]; res[pn + 15 * n_imu + 2 * f + 1] = r[1]; }
        if (bc) bc[1 + n_imu + f] = c;
        if (want_g) {
            gbl_d *o = pc_proj + f * EV_PIECE_PROJ;
            for (int j = 0; j < 20; j++) o[j] = j < ncol ? J[j] * r[0] + J[20 + j] * r[1] : 0.0;
        }
    }
    const double fam_proj = ev_block_sum(part, red, tid);

    // ---- line factors (line_projection_factor.cpp:19-120)
    part = 0.0;
    for (int f = tid; f < n_line; f += 256) {
        const lds_d *xp = x + blk[ip[P.o_line + f] * 4 + 1];
        double r[2], J[12], ld9[9], lc[21];
#pragma unroll
        for (int i = 0; i < 9; i++) ld9[i] = dp[W->d_line + f * 9 + i];
#pragma unroll
        for (int i = 0; i < 21; i++) lc[i] = dp[W->d_linec + i];
        line_eval(CGEN(xp), ld9, lc, lc + 9, lc + 18, r, want_g ? J : nullptr, 6, misc[8] != 0.0);
        const double c = loss_correct2(r, want_g ? J : nullptr, 6, 6, line_loss);
        part += c;
        if (res) { res[pn + 15 * n_imu + 2 * n_proj + 2 * f] = r[0]; res[pn + 15 * n_imu + 2 * n_proj + 2 * f + 1] = r[1]; }
        if (bc) bc[1 + n_imu + n_proj + f] = c;
        if (want_g) {
            gbl_d *o = pc_line + f * EV_PIECE_LINE;
            for (int j = 0; j < 6; j++) o[j] = J[j] * r[0] + J[6 + j] * r[1];
        }
    }
    const double fam_line = ev_block_sum(part, red, tid);      // (its barriers also order the pieces in HBM before the owners read them)

    // ---- gradient: every tangent index is added by its owner thread, its pieces in factor order
    double gmax = -1.0;
    if (want_g) {
        __threadfence_block();
        __syncthreads();
        gbl_d *g = (gbl_d *)(A.gradient + (size_t)win * A.grad_stride);
        const int *tab = A.tab + A.tab_base[W->plan];
        const int *items = tab + nc + L + 1;
        double m = 0.0;
        for (int t = tid; t < nc + L; t += 256) {
            double acc = 0.0;
            for (int e = tab[t]; e < tab[t + 1]; e++) acc += piece[items[e]];
            g[t] = acc;
            m = ev_max_nan(fabs(acc), m);
        }
        red[tid] = m;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] = ev_max_nan(red[tid], red[tid + s]);
            __syncthreads();
        }
        gmax = red[0];
    }
    if (tid == 0) {
        gbl_d *o = (gbl_d *)(A.scalars + (size_t)win * EV_SCALARS);
        o[EV_FAMILY] = fam_prior; o[EV_FAMILY + 1] = fam_imu; o[EV_FAMILY + 2] = fam_proj; o[EV_FAMILY + 3] = fam_line;
        o[EV_COST] = ((fam_prior + fam_imu) + fam_proj) + fam_line;
        o[EV_GMAX] = gmax;
    }
}

}  // namespace tcv

extern "C" int tcv_launch_evaluate(const tcv::EvalArgs *args, size_t lds_bytes, void *stream) {
    using namespace tcv;
    hipLaunchKernelGGL(evaluate_kernel, dim3(args->nwin), dim3(256), lds_bytes, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
// registers, LDS and resident workgroups per CU of the kernel (tools/dev_evaluate_bench.py): out4 = VGPRs, static + dynamic LDS bytes,
// scratch bytes per thread, workgroups per CU the runtime reports for that LDS size
extern "C" int tcv_evaluate_kernel_shape(size_t lds_bytes, int *out4) {
    using namespace tcv;
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, (const void *)evaluate_kernel);
    if (e != hipSuccess) return (int)e;
    int nb = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)evaluate_kernel, 256, lds_bytes);
    if (e != hipSuccess) return (int)e;
    out4[0] = fa.numRegs; out4[1] = (int)(fa.sharedSizeBytes + lds_bytes); out4[2] = (int)fa.localSizeBytes; out4[3] = nb;
    return 0;
}
