// tcv::covariance_kernel -- ceres::Covariance::Compute + GetCovarianceBlockInTangentSpace for every window of a resident batch: the
// requested blocks of S^-1, S = H_cc - sum_l h_l h_l' / H_ll the reduced camera system of H = J'J (loss-corrected Jacobians and the
// prior's J0) at either the uploaded initial states or the states the last solve left.  It reads the batch as the evaluation kernel
// does (tcv_packed.h) and uses the same factor code (tcv_factors.h); nothing of the solve / marginalisation / evaluation kernels is touched.
//
// One 256-thread workgroup per window at a time (a persistent grid walks the batch), FP64 throughout:
//   1. states in LDS; every factor leaves its tangent-space Jacobian in the workgroup's staging area (HBM, L2-resident)
//   2. per landmark 1 / H_ll and its coupling vector h_l, each entry summed by one thread in plan order, in twice the working precision
//   3. S entry by entry into LDS (packed lower triangle, row-major: 183 * 184 / 2 doubles = 135 KB): every entry is summed by ONE owner
//      in the order of its host-built owner list (tcv_cov.h) -- prior, IMU, point, line, landmarks -- in twice the working precision
//      (dd_fma below) and rounded once.  No atomics; the order depends on the
//      window alone, never on the batch, the grid or the timing
//   4. left-looking Cholesky in place, one row per thread, dot products in twice the working precision, with the rank gate per pivot
//      (tcv_cov.h cov_pivot_status)
//   5. one thread per requested unit column e_p: y_p = L^-1 e_p by forward substitution (L in LDS, y in HBM)
//   6. the requested entries (S^-1)_pq = y_p . y_q, summed in ascending row order (steps 5 and 6 in twice the working precision too) -- the backward substitution folded into a dot product,
//      which makes block (i, j) the exact transpose of block (j, i) and every diagonal block exactly symmetric
//   7. (LM instantiation only: tcv_batch_compute_landmark_covariance) the inverse depths, in chunks of COV_LM_CHUNK landmarks, one
//      thread per landmark: w_l = h_l / H_ll scattered into tangent order, y_l = L^-1 w_l by forward substitution from the first
//      non-zero row (L in LDS, y_l in HBM), var = 1 / H_ll + sum_k y_l[k]^2, k ascending; then cov(lambda_l, column p) = -sum_k y_l[k] y_p[k]
//      for the columns step 5 solved, one thread per entry.  Every sum in twice the working precision; the dot products of the substitution
//      and of the cross entries as four interleaved partial sums (dd_dot4 below): an order that depends on the plan alone
// A window that fails the gate gets status 1 (2: NaN / Inf) and zero blocks.
#include <hip/hip_runtime.h>

#include "tcv_cov.h"
#include "tcv_dev.h"
#include "tcv_factors.h"

namespace tcv {

// Sums in twice the working precision (Ogita, Rump, Oishi: Dot2): hi + lo carries the running sum, every product enters with its exact
// rounding error (FMA) and every addition with its own (TwoSum).  The entries of S are differences of large sums -- the landmarks take
// most of what the point factors give the extrinsic and the anchor poses -- and a plain serial sum over ~2000 terms loses there what the
// factorisation cannot give back.  Each operation is a statement of its own: -ffp-contract=on fuses within an expression only.
__device__ __forceinline__ void dd_add(double &hi, double &lo, double p, double pe) {
    const double s = hi + p;
    const double bb = s - hi;
    const double se = (hi - (s - bb)) + (p - bb);
    hi = s;
    lo += se + pe;
}
__device__ __forceinline__ void dd_fma(double &hi, double &lo, double a, double b) {
    const double p = a * b;
    const double pe = __builtin_fma(a, b, -p);
    dd_add(hi, lo, p, pe);
}

// init + sum_{k0 <= k < k1} a(k) b(k) for phase 7, in twice the working precision and rounded once, as four interleaved partial sums: the
// operands of a group are loaded before its first product, so that a group costs one round trip to the y buffers, not one per term, and
// four chains run side by side.  Groups of eight, then one of four, go to partial sums 0 .. 3 in turn; a tail of up to three terms goes to
// partial sum 0; the partial sums are added as (0 + 1) + (2 + 3).  The order depends on k0 and k1 alone.
template <class FA, class FB> __device__ __forceinline__ double dd_dot4(double init, int k0, int k1, FA a, FB b) {
    double h0 = init, l0 = 0.0, h1 = 0.0, l1 = 0.0, h2 = 0.0, l2 = 0.0, h3 = 0.0, l3 = 0.0;
    int k = k0;
    for (; k + 7 < k1; k += 8) {
        const double a0 = a(k), a1 = a(k + 1), a2 = a(k + 2), a3 = a(k + 3), a4 = a(k + 4), a5 = a(k + 5), a6 = a(k + 6), a7 = a(k + 7);
        const double b0 = b(k), b1 = b(k + 1), b2 = b(k + 2), b3 = b(k + 3), b4 = b(k + 4), b5 = b(k + 5), b6 = b(k + 6), b7 = b(k + 7);
        dd_fma(h0, l0, a0, b0); dd_fma(h1, l1, a1, b1); dd_fma(h2, l2, a2, b2); dd_fma(h3, l3, a3, b3);
        dd_fma(h0, l0, a4, b4); dd_fma(h1, l1, a5, b5); dd_fma(h2, l2, a6, b6); dd_fma(h3, l3, a7, b7);
    }
    if (k + 3 < k1) {
        const double a0 = a(k), a1 = a(k + 1), a2 = a(k + 2), a3 = a(k + 3), b0 = b(k), b1 = b(k + 1), b2 = b(k + 2), b3 = b(k + 3);
        dd_fma(h0, l0, a0, b0); dd_fma(h1, l1, a1, b1); dd_fma(h2, l2, a2, b2); dd_fma(h3, l3, a3, b3);
        k += 4;
    }
    for (; k < k1; k++) dd_fma(h0, l0, a(k), b(k));
    dd_add(h0, l0, h1, l1);
    dd_add(h2, l2, h3, l3);
    dd_add(h0, l0, h2, l2);
    return h0 + l0;
}

template <bool LM> __global__ void __launch_bounds__(256) covariance_kernel(CovArgs A) {
    extern __shared__ __attribute__((aligned(16))) double cov_lds_raw[];
    const int tid = threadIdx.x;
    lds_d *lds = (lds_d *)cov_lds_raw;
    lds_d *x = lds, *red = x + A.state_stride, *pdx = red + 256, *pr = pdx + 128, *ws = pr + 128;      // phase 1
    lds_d *tri = lds, *pivot = lds + A.lds_area, *ldiag = pivot + 2;                                  // phases 3 - 6
    gbl_d *stage = (gbl_d *)(A.stage + (size_t)blockIdx.x * A.stage_stride);
    gbl_d *Y = (gbl_d *)(A.ybuf + (size_t)blockIdx.x * COV_MAX_DIM * COV_MAX_DIM);

    for (int win = blockIdx.x; win < A.nwin; win += gridDim.x) {
        cst_win *W = (cst_win *)(A.win + win);
        cst_plan &P = *(cst_plan *)(A.plans + W->plan);
        cst_i *ip = (cst_i *)(A.ipool + A.plan_base[W->plan]);
        cst_d *dp = (cst_d *)(A.dpool + W->dbase);
        cst_i *blk = ip + P.o_blk;
        cst_d *misc = dp + W->d_misc;
        const int nx = P.nx, L = P.nland, nc = P.nc, n_imu = P.n_imu, n_proj = P.n_proj, n_line = P.n_line, pn = P.prior_n;
        const int *tab = A.tab + A.tab_base[W->plan];
        const int *rq = A.rq + (size_t)win * A.rq_stride;
        gbl_d *g_sqrt = stage, *g_rec = g_sqrt + n_imu * 225, *Jr = g_rec + n_imu * IMU_REC;
        gbl_d *j_imu = Jr, *j_proj = Jr + tab[CT_JPROJ], *j_line = Jr + tab[CT_JLINE], *j_hll = Jr + tab[CT_JHLL];
        gbl_d *out = (gbl_d *)(A.out + (size_t)win * A.n_req * COV_BLOCK_DOUBLES);

        // ---- 1. the evaluation point and the Jacobians
        if (A.state) { const double *s = A.state + (size_t)win * A.state_stride; for (int i = tid; i < nx + L; i += 256) x[i] = s[i]; }
        else for (int i = tid; i < nx + L; i += 256) x[i] = dp[W->d_x + i];
        __syncthreads();
        if (n_imu > 0) {      // imu_factor.h:19-181: sqrt_info (given, or LLT(cov^-1).matrixL()^T on the device), raw record, whitening
            if (W->d_sqrt >= 0) {
                for (int i = tid; i < n_imu * 225; i += 256) g_sqrt[i] = dp[W->d_sqrt + i];
            } else {
                for (int f0 = 0; f0 < n_imu; f0 += 8) {
                    const int grp = tid >> 4, f = f0 + grp;
                    if (grp < 8 && f < n_imu)
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
                                 cst, G3, GEN(g_rec + lane * IMU_REC), IMU_STRIDE_J, true);
                }
            }
            __threadfence_block();
            __syncthreads();
            for (int q = tid; q < n_imu * COV_J_IMU; q += 256) {      // J = sqrt_info * J_raw
                const int f = q / COV_J_IMU, e = q - COV_J_IMU * f, i = e / 30, c = e - 30 * i;
                const gbl_d *S = g_sqrt + f * 225 + i * 15, *Jc = g_rec + f * IMU_REC + c;
                double v = 0.0;
                for (int k = 0; k < 15; k++) v += S[k] * Jc[k * IMU_STRIDE_J];
                j_imu[q] = v;
            }
        }
        // point factors (projection_factor.cpp:21-124, projection_td_factor.cpp:34-140), in plan order
        const double proj_sqrt = misc[3], proj_loss = A.apply_loss ? misc[4] : 0.0, line_loss = A.apply_loss ? misc[5] : 0.0;
        const bool with_td = (P.flags & 1) != 0;
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
                proj_td_eval(CGEN(xi), CGEN(xj), CGEN(xe), lam, tdv, pts, aux, proj_sqrt, misc[6], misc[7], r, J, 20);
                ncol = 20;
            } else {
                proj_eval(CGEN(xi), CGEN(xj), CGEN(xe), lam, pts, proj_sqrt, r, J, 20);
                J[19] = 0.0; J[39] = 0.0;
            }
            (void)loss_correct2(r, J, ncol, 20, proj_loss);
            gbl_d *o = j_proj + f * COV_J_PROJ;
            for (int j = 0; j < 40; j++) o[j] = J[j];
        }
        // line factors (line_projection_factor.cpp:19-120)
        for (int f = tid; f < n_line; f += 256) {
            const lds_d *xp = x + blk[ip[P.o_line + f] * 4 + 1];
            double r[2], J[12], ld9[9], lc[21];
#pragma unroll
            for (int i = 0; i < 9; i++) ld9[i] = dp[W->d_line + f * 9 + i];
#pragma unroll
            for (int i = 0; i < 21; i++) lc[i] = dp[W->d_linec + i];
            line_eval(CGEN(xp), ld9, lc, lc + 9, lc + 18, r, J, 6, misc[8] != 0.0);
            (void)loss_correct2(r, J, 6, 6, line_loss);
            gbl_d *o = j_line + f * COV_J_LINE;
            for (int j = 0; j < 12; j++) o[j] = J[j];
        }
        __threadfence_block();
        __syncthreads();      // the states in LDS are dead from here on

        // ---- 2. landmarks: 1 / H_ll, then h_l slot by slot (8 lanes per slot)
        {
            const int *lmptr = tab + tab[CT_OLMPTR], *lmfac = tab + tab[CT_OLMFAC];
            for (int l = tid; l < L; l += 256) {
                double h = 0.0, hl = 0.0;
                for (int e = lmptr[l]; e < lmptr[l + 1]; e++) {
                    const gbl_d *o = j_proj + lmfac[e] * COV_J_PROJ;
                    dd_fma(h, hl, o[18], o[18]);
                    dd_fma(h, hl, o[38], o[38]);
                }
                const double d = h + hl, dl = (h - d) + hl;      // H_ll = d + dl; its reciprocal ih + il
                const double ih = d > 0.0 ? 1.0 / d : 0.0;
                const double r = __builtin_fma(-d, ih, 1.0) - dl * ih;
                j_hll[2 * l] = ih;
                j_hll[2 * l + 1] = d > 0.0 ? r * ih : 0.0;
            }
            const int nh = tab[CT_NHSLOT], *hs = tab + tab[CT_OHSLOT], *hi = tab + tab[CT_OHITEM];
            for (int s = tid >> 3; s < nh; s += 32) {
                const int j = tid & 7, *q = hs + s * CT_HSLOT;
                if (j >= q[1]) continue;
                double h = 0.0, hl = 0.0;
                for (int e = q[2]; e < q[3]; e++) {
                    const int o = hi[e * CT_HITEM] + j, ol = hi[e * CT_HITEM + 1];
                    dd_fma(h, hl, Jr[o], Jr[ol]);
                    dd_fma(h, hl, Jr[o + 20], Jr[ol + 20]);
                }
                const double hh = h + hl;
                Jr[q[0] + j] = hh;
                Jr[q[0] + 6 + j] = (h - hh) + hl;
            }
        }
        __threadfence_block();
        __syncthreads();

        // ---- 3. S: the entries no pair owns are exact zeros; wave w owns pairs w, w + 4, ...
        for (int i = tid; i < nc * (nc + 1) / 2; i += 256) tri[i] = 0.0;
        __syncthreads();
        {
            const int npair = tab[CT_NPAIR], *pairs = tab + tab[CT_OPAIR], *items = tab + tab[CT_OITEM];
            const int k0 = W->prior_k0, nr = pn - k0;
            cst_d *J0 = dp + W->d_prior;
            const int lane = tid & 63;
            for (int p = tid >> 6; p < npair; p += 4) {
                const int *q = pairs + p * CT_PAIR;
                const int ta = q[0], tb = q[1], wa = q[2], wb = q[3], pca = q[6], pcb = q[7];
                for (int e = lane; e < wa * wb; e += 64) {
                    const int i = e / wb, j = e - wb * i;
                    if (ta + i < tb + j) continue;      // (the upper half of a diagonal pair)
                    double acc = 0.0, lo = 0.0;
                    if (pca >= 0 && pn > 0) {
                        cst_d *ca = J0 + (size_t)nr * (pca + i), *cb = J0 + (size_t)nr * (pcb + j);
                        for (int r = 0; r < nr; r++) dd_fma(acc, lo, ca[r], cb[r]);
                    }
                    for (int it = q[4]; it < q[5]; it++) {
                        const int *d = items + it * CT_ITEM;
                        const gbl_d *a = Jr + d[0] + i, *b = Jr + d[1] + j;
                        if (d[3] >= 0) {      // - (h_a h_b) / H_ll, every factor hi + lo
                            const double ah = a[0], al = a[6], bh = b[0], bl = b[6], ih = Jr[d[3]], il = Jr[d[3] + 1];
                            const double ph = ah * bh;
                            const double cross = ah * bl + al * bh;
                            const double pl = __builtin_fma(ah, bh, -ph) + cross;
                            const double t = ph * ih;
                            const double rest = ph * il + pl * ih;
                            const double tl = __builtin_fma(ph, ih, -t) + rest;
                            dd_add(acc, lo, -t, -tl);
                        } else {
                            const int rows = d[2] >> 16, rs = d[2] & 0xffff;
                            for (int r = 0; r < rows; r++) dd_fma(acc, lo, a[r * rs], b[r * rs]);
                        }
                    }
                    tri[(ta + i) * (ta + i + 1) / 2 + tb + j] = acc + lo;
                }
            }
        }
        __syncthreads();

        // ---- 4. Cholesky, left-looking, one row per thread: L_ij = (S_ij - sum_{k < j} L_ik L_jk) / L_jj with the sum in twice the working
        // precision, subtracted from S_ij once.  (The right-looking form subtracts term by term from entries of 2e15 -- the bias random
        // walk -- whose pivots end near 1e5: it lost a digit and more against this one.)  The diagonal of `tri` keeps S_jj for the gate;
        // every thread takes the same decision.
        int st = COV_STATUS_OK;
        for (int j = 0; j < nc; j++) {
            const int i = j + tid;
            double s = 0.0;
            if (i < nc) {
                const lds_d *ri = tri + i * (i + 1) / 2, *rj = tri + j * (j + 1) / 2;
                double hi = ri[j], lo = 0.0;
                for (int k = 0; k < j; k++) dd_fma(hi, lo, -ri[k], rj[k]);
                s = hi + lo;
            }
            if (tid == 0) pivot[0] = s;
            __syncthreads();
            const double d = pivot[0];
            st = cov_pivot_status(d, tri[j * (j + 1) / 2 + j], A.min_relative_pivot);
            if (st != COV_STATUS_OK) break;
            const double ljj = sqrt(d);
            if (tid == 0) ldiag[j] = ljj;
            else if (i < nc) tri[i * (i + 1) / 2 + j] = s / ljj;
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) A.status[win] = st;
        const int m = rq[RQ_M], n_req = rq[RQ_NREQ];
        if (st != COV_STATUS_OK) {
            for (int i = tid; i < n_req * COV_BLOCK_DOUBLES; i += 256) out[i] = 0.0;
            if (LM) {
                gbl_d *lv = (gbl_d *)(A.lm_var + (size_t)win * A.lm_lmax), *lc = (gbl_d *)(A.lm_cross + (size_t)win * A.lm_lmax * A.lm_mstride);
                for (int i = tid; i < L; i += 256) lv[i] = 0.0;
                for (int i = tid; i < L * A.lm_mstride; i += 256) lc[i] = 0.0;
            }
            __syncthreads();
            continue;
        }

        // ---- 5. y_p = L^-1 e_p, one thread per solved column
        if (tid < m) {
            const int t = rq[RQ_COL + tid];
            Y[t * m + tid] = 1.0 / ldiag[t];
            for (int i = t + 1; i < nc; i++) {
                const lds_d *row = tri + i * (i + 1) / 2;
                double hi = 0.0, lo = 0.0;
                for (int k = t; k < i; k++) dd_fma(hi, lo, row[k], Y[k * m + tid]);
                Y[i * m + tid] = -(hi + lo) / ldiag[i];
            }
        }
        __threadfence_block();
        __syncthreads();

        // ---- 6. the requested blocks: (S^-1)_pq = sum_k y_p[k] y_q[k], k ascending from max(p, q)
        for (int e = tid; e < n_req * COV_BLOCK_DOUBLES; e += 256) {
            const int r = e / COV_BLOCK_DOUBLES, c = e - COV_BLOCK_DOUBLES * r;
            const int *q = rq + RQ_REQ + 4 * r;
            const int ci = q[0], wi = q[1], cj = q[2], wj = q[3];
            double v = 0.0, lo = 0.0;
            if (ci >= 0 && cj >= 0 && c < wi * wj) {
                const int a = c / wj, b = c - wj * a;
                const int p = rq[RQ_COL + ci + a], s = rq[RQ_COL + cj + b];
                for (int k = p > s ? p : s; k < nc; k++) dd_fma(v, lo, Y[k * m + ci + a], Y[k * m + cj + b]);
            }
            out[e] = v + lo;
        }

        // ---- 7. the landmarks, COV_LM_CHUNK at a time: one thread per landmark for y_l and the variance, then one thread per cross entry
        if (LM) {
            const int *lt = A.ltab + A.ltab_base[W->plan], *lslot = lt + L + 1;
            gbl_d *YL = (gbl_d *)(A.ylm + (size_t)blockIdx.x * COV_MAX_DIM * COV_LM_CHUNK);
            gbl_d *lvar = (gbl_d *)(A.lm_var + (size_t)win * A.lm_lmax), *lcross = (gbl_d *)(A.lm_cross + (size_t)win * A.lm_lmax * A.lm_mstride);
            for (int l0 = 0; l0 < L; l0 += COV_LM_CHUNK) {
                const int nl = L - l0 < COV_LM_CHUNK ? L - l0 : COV_LM_CHUNK;
                if (tid < nl) {
                    const int l = l0 + tid, s0 = lt[l], s1 = lt[l + 1];
                    const int t0 = s1 > s0 ? lslot[s0 * LT_SLOT] : nc;
                    const double ih = j_hll[2 * l], il = j_hll[2 * l + 1];
                    for (int k = t0; k < nc; k++) YL[k * COV_LM_CHUNK + tid] = 0.0;
                    for (int s = s0; s < s1; s++) {      // w = (h hi + lo) * (1 / H_ll hi + lo), rounded once
                        const int *q = lslot + s * LT_SLOT;
                        for (int j = 0; j < q[2]; j++) {
                            const double hh = Jr[q[1] + j], hl = Jr[q[1] + 6 + j];
                            const double t = hh * ih;
                            const double rest = hh * il + hl * ih;
                            const double tl = __builtin_fma(hh, ih, -t) + rest;
                            YL[(q[0] + j) * COV_LM_CHUNK + tid] = t + tl;
                        }
                    }
                    double vh = ih, vl = il;
                    for (int i = t0; i < nc; i++) {
                        const lds_d *row = tri + i * (i + 1) / 2;
                        const double y = dd_dot4(YL[i * COV_LM_CHUNK + tid], t0, i, [&](int k) { return -row[k]; }, [&](int k) { return YL[k * COV_LM_CHUNK + tid]; }) / ldiag[i];
                        YL[i * COV_LM_CHUNK + tid] = y;
                        dd_fma(vh, vl, y, y);
                    }
                    lvar[l] = vh + vl;
                }
                __threadfence_block();
                __syncthreads();
                for (int e = tid; e < nl * m; e += 256) {
                    const int c = e / nl, t = e - nl * c, l = l0 + t;
                    const int s0 = lt[l], t0 = lt[l + 1] > s0 ? lslot[s0 * LT_SLOT] : nc, p = rq[RQ_COL + c];
                    // (0.0 - x, not -x: an empty sum -- a landmark all of whose slots are constant -- is +0.0, like every other zero this call returns)
                    lcross[(size_t)l * A.lm_mstride + c] = 0.0 - dd_dot4(0.0, t0 > p ? t0 : p, nc, [&](int k) { return YL[k * COV_LM_CHUNK + t]; }, [&](int k) { return Y[k * m + c]; });
                }
                __syncthreads();      // the chunk's y_l go to the next chunk
            }
        }
        __syncthreads();      // LDS and the staging area go to the next window
    }
}

}  // namespace tcv

// covariance_kernel<true> carries the landmark phase (tcv_batch_compute_landmark_covariance); the plain call's kernel is covariance_kernel<false>
extern "C" int tcv_launch_covariance(const tcv::CovArgs *args, int grid, size_t lds_bytes, void *stream, bool landmarks) {
    using namespace tcv;
    const auto kernel = !landmarks ? covariance_kernel<false> : covariance_kernel<true>;      // (instantiated in this order: the code object keeps its layout)
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_bytes, (hipStream_t)stream, *args);
    return (int)hipGetLastError();
}
