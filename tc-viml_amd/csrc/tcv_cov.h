// Arguments and side tables of tcv::covariance_kernel (tcv_cov.hip): ceres::Covariance for every window of a resident batch -- the
// marginal covariance S^-1 of the camera-side states, S = H_cc - sum_l h_l h_l' / H_ll the reduced camera system of H = J'J at the
// evaluation point.  The kernel reads what the batch holds already (window headers, plans, pools of tcv_packed.h) plus two side tables
// that live BESIDE the plans: the owner lists of S (one per distinct plan, built once per batch) and the request table (one per window,
// rebuilt when the request list changes).  Host half: tcv_cov_tables.cpp builds the tables, tcv_cov_host.cpp keeps the buffers.
#pragma once
#include "tcv_packed.h"

namespace tcv {

enum { COV_MAX_DIM = 184, COV_BLOCK_DOUBLES = 81 };
enum { COV_STATUS_OK = 0, COV_STATUS_RANK = 1, COV_STATUS_NONFINITE = 2 };

// ---- the staging area of one workgroup (doubles, CovArgs::stage)
//   [ sqrt_info of the IMU factors 225 each | their raw records IMU_REC each | J region ]
// The J region holds every factor's tangent-space Jacobian as the owners of S read it (offsets below are relative to its start):
//   [ IMU: 15 x 30 whitened, row-major | point: 2 x 20 loss-corrected (pose_i 6, pose_j 6, ex 6, inverse depth, td) in plan order |
//     line: 2 x 6 | 1 / H_ll per landmark as hi, lo (0: no information) | h_l: per landmark its slots, 6 doubles hi + 6 doubles lo
//     each (a td slot uses 1 of either) ]
// h_l and 1 / H_ll are kept as unevaluated sums hi + lo of two doubles: the owners of S add in twice the working precision (tcv_cov.hip)
enum { COV_J_IMU = 450, COV_J_PROJ = 40, COV_J_LINE = 12, COV_SLOT = 12 };

// ---- owner lists of S, per plan (ints, CovArgs::tab + tab_base[plan]): a header, then the arrays it points to (offsets relative to the header)
//   pair  (8 ints): ta, tb (first tangent index of the two blocks, ta >= tb), wa, wb, item_begin, item_end, pca, pcb (first prior column
//                   of either block when BOTH are in the prior, else -1)
//   item  (4 ints): offA, offB (J-region offsets of row 0 of the two column blocks), rows << 16 | row stride, sc
//                   sc < 0 : S(ta + i, tb + j) += sum_rows J[offA + row * stride + i] * J[offB + row * stride + j]
//                   sc >= 0: a landmark: S(ta + i, tb + j) -= h[offA + i] * h[offB + j] * J[sc]       (J[sc], J[sc + 1] = 1 / H_ll)
//   The owner of an entry adds the prior's J0'J0 first, then its pair's items in list order: IMU factors, point factors in plan order,
//   line factors, then the landmarks in plan order.  The lists are a function of the plan alone: the same bits whatever the batch.
//   hslot (4 ints): offset of the slot in the J region, width, hitem_begin, hitem_end;  hitem (2 ints): offsets of J(0, first column of
//   the block) and J(0, inverse depth) of one point factor: h[j] = sum_items J[o + j] * J[ol] + J[o + 20 + j] * J[ol + 20]
//   lmptr (nland + 1) / lmfac: the point factors (plan order) of every landmark: H_ll = sum J[18]^2 + J[38]^2
enum {
    CT_NPAIR = 0, CT_OPAIR, CT_OITEM, CT_NHSLOT, CT_OHSLOT, CT_OHITEM, CT_OLMPTR, CT_OLMFAC, CT_JPROJ, CT_JLINE, CT_JHLL, CT_JDOUBLES,
    CT_HDR = 16, CT_PAIR = 8, CT_ITEM = 4, CT_HSLOT = 4, CT_HITEM = 2
};
// ---- request table, per window (ints, CovArgs::rq + window * rq_stride):
//   [ m (solved columns) | n_req | tangent index of every solved column (COV_MAX_DIM) | per request ci, wi, cj, wj ]
//   ci / cj: first solved column of block i / j (-1: a constant block, the request's block is zero)
enum { RQ_M = 0, RQ_NREQ = 1, RQ_COL = 2, RQ_REQ = 2 + COV_MAX_DIM };
inline int cov_rq_stride(int n_req) { return RQ_REQ + 4 * n_req; }

// ---- landmark phase (include/tcv_landmark_covariance.h; tcv_cov.hip phase 7), only in the instantiation the landmark call launches.
// Slot table, per plan (ints, CovArgs::ltab + ltab_base[plan]), beside the owner lists:
//   [ lsptr (nland + 1) | slot (3 ints): first tangent index of the block, offset of its h_l slot in the J region, width ]
//   the slots of landmark l are lsptr[l] .. lsptr[l + 1], in ascending tangent order: the first one is the first non-zero row of w_l
// The landmarks are walked in chunks of COV_LM_CHUNK, one thread per landmark; y_l = L^-1 w_l of a chunk lives in the workgroup's
// CovArgs::ylm (COV_MAX_DIM x COV_LM_CHUNK: row k of landmark t at k * COV_LM_CHUNK + t).
// Results, landmarks in plan order: CovArgs::lm_var + window * lm_lmax: var(lambda_l);  CovArgs::lm_cross + window * lm_lmax * lm_mstride:
// rows of lm_mstride doubles, row l, entry c = cov(lambda_l, solved column c of the window's request table) -- the host cuts the
// requested blocks out of the rows
enum { COV_LM_CHUNK = 256, LT_SLOT = 3 };

// LDS doubles of a workgroup: first the evaluation phase (states | reduction scratch | prior dx | prior residual | sqrt_info workspace, as
// tcv_eval.h), then -- over the same space -- the packed lower triangle of S, row-major (its diagonal keeps S_kk); behind it the pivot
// of the current column and diag(L)
inline int cov_lds_area(int state_stride, int nc_max) { const int a = state_stride + 256 + 128 + 128 + 8 * 450, t = nc_max * (nc_max + 1) / 2; return ((a > t ? a : t) + 1) & ~1; }
inline int cov_lds_doubles(int state_stride, int nc_max) { return cov_lds_area(state_stride, nc_max) + 2 + COV_MAX_DIM; }

// Rank gate of pivot k (include/tcv_covariance.h min_relative_pivot): d = the pivot before its square root (L_kk^2), s = S_kk.
// 0 fine, COV_STATUS_RANK: d <= min_rel * s, COV_STATUS_NONFINITE: NaN / Inf in either.
__host__ __device__ inline int cov_pivot_status(double d, double s, double min_rel) {
    if (!(d - d == 0.0) || !(s - s == 0.0)) return COV_STATUS_NONFINITE;
    return d > min_rel * s ? COV_STATUS_OK : COV_STATUS_RANK;
}

struct CovArgs {
    const WinHdr *win;
    const PlanHdr *plans;
    const long long *plan_base;
    const int *ipool;
    const double *dpool;
    const double *state;          // null: the uploaded initial states; else per window nx + nland (stride state_stride)
    const long long *tab_base;    // per plan: offset of its owner lists in `tab`
    const int *tab;
    const int *rq;                // per window rq_stride ints
    double *stage;                // per workgroup (stride stage_stride)
    double *ybuf;                 // per workgroup COV_MAX_DIM x COV_MAX_DIM: L^-1 E, row k of column c at k * m + c
    double *out;                  // per window n_req x COV_BLOCK_DOUBLES, block k row-major at k * COV_BLOCK_DOUBLES
    int *status;                  // per window
    long long stage_stride;
    int nwin, state_stride, rq_stride, n_req;
    int apply_loss, lds_area;
    double min_relative_pivot;
    // landmark phase (null / 0 in the plain call)
    const long long *ltab_base;   // per plan: offset of its slot table in `ltab`
    const int *ltab;
    double *ylm;                  // per workgroup COV_MAX_DIM x COV_LM_CHUNK
    double *lm_var, *lm_cross;    // per window lm_lmax / lm_lmax x lm_mstride
    int lm_lmax, lm_mstride;      // largest landmark count / largest number of solved columns of the batch
};

}  // namespace tcv
