// Arguments of tcv::evaluate_kernel (tcv_eval.hip): ceres::Problem::Evaluate for every window of a resident batch.
// The kernel reads what the batch holds already (window headers, plans, int / double pools of tcv_packed.h) plus one side table per
// distinct plan that lives BESIDE the plan, not in it: the owner lists of the gradient.
#pragma once
#include "tcv_packed.h"

namespace tcv {

// per-window scalar block written by the kernel (doubles)
enum { EV_COST = 0, EV_FAMILY = 1, EV_GMAX = 5, EV_SCALARS = 8 };
// Staging area of one window (doubles, EvalArgs::stage): sqrt_info of the IMU factors, their raw records [J_raw | r_raw], then the J'r
// PIECES every factor leaves for the owner threads of the gradient:
//   [ prior: n (J0' r per column) | IMU: 30 per factor (local columns of tcv_factors.h) | point: 20 per factor (pose_i 6, pose_j 6, ex 6,
//     inverse depth, td) in plan order | line: 6 per factor ]
// The owner list of tangent index t (camera tangent space, then the landmarks: nc + nland entries) holds the offsets of its pieces in that
// region in factor order; the owner adds them in that order: no atomics, the same bits whatever the batch.
enum { EV_PIECE_IMU = 30, EV_PIECE_PROJ = 20, EV_PIECE_LINE = 6, EV_SQRT_ROUND = 8 };
inline int eval_piece_doubles(const PlanHdr &H) { return H.prior_n + EV_PIECE_IMU * H.n_imu + EV_PIECE_PROJ * H.n_proj + EV_PIECE_LINE * H.n_line; }
inline int eval_stage_doubles(const PlanHdr &H) { return H.n_imu * (225 + IMU_REC) + eval_piece_doubles(H); }
inline int eval_num_residuals(const PlanHdr &H) { return H.prior_n + 15 * H.n_imu + 2 * H.n_proj + 2 * H.n_line; }
inline int eval_num_blocks(const PlanHdr &H) { return 1 + H.n_imu + H.n_proj + H.n_line; }      // slot 0: the prior (0 without one)
// LDS doubles of a workgroup: states | reduction scratch | prior dx | prior residual | sqrt_info workspace (EV_SQRT_ROUND factors at a time)
inline int eval_lds_doubles(int state_stride) { return state_stride + 256 + 128 + 128 + EV_SQRT_ROUND * 450; }

struct EvalArgs {
    const WinHdr *win;
    const PlanHdr *plans;
    const long long *plan_base;
    const int *ipool;
    const double *dpool;
    const double *state;          // null: the uploaded initial states (WinHdr::d_x); else per window nx + nland (stride state_stride)
    const long long *tab_base;    // per plan: offset of its owner lists in `tab`: [ptr (nc + nland + 1) | piece offsets]
    const int *tab;
    double *scalars;              // per window EV_SCALARS
    double *residuals;            // optional, per window (stride res_stride): prior rows, IMU, point (plan order), line
    double *block_cost;           // optional, per window (stride blk_stride): prior, IMU, point (plan order), line
    double *gradient;             // optional, per window (stride grad_stride): camera tangent space, then the landmarks
    double *stage;                // per window (stride stage_stride)
    int nwin, state_stride, res_stride, blk_stride, grad_stride, stage_stride;
    int apply_loss, pad;
};

}  // namespace tcv
