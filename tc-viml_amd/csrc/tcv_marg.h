// What the marginalisation kernel (tcv_marg.hip) and its host side (tcv_marg_host.cpp) share: the limits, the layout of the per-window
// result block and scratch, the plan header the packer writes and the kernel reads, and the launchers.
#pragma once
#include "tcv_host.h"

namespace tcv {

enum { MARG_MAX_M = 64, MARG_MAX_N = 80, MARG_MAX_POS = MARG_MAX_M + MARG_MAX_N, MARG_MAX_X = 1408 };
// Two launch shapes of the one kernel: 512 threads per window and one workgroup per CU (few windows: shortest time per window), or
// 256 threads per window and two workgroups per CU when every window of the batch fits 80 KB of LDS (many windows: the barrier and
// LDS round trips of one window hide behind the other's arithmetic).
enum { MARG_SM_DOUBLES = 720 };
enum { MARG_NT_WIDE = 512, MARG_NT_PAIR = 256, MARG_SM = MARG_SM_DOUBLES, MARG_STAGE = 64 * 43, MARG_CB_LM = 16 };
// per-window result block: [J0 | r0 | x (linearisation point) + 64 diagnostics] is what a caller needs (MARG_OUT_COMPACT doubles, the
// part tcv_batch_download_priors_compact copies); A', b' (parity / debug surface) follow
enum { MARG_OUT_J0 = 0, MARG_OUT_R0 = 6400, MARG_OUT_X = 6480, MARG_OUT_COMPACT = 6480 + 1408 + 64, MARG_OUT_AS = MARG_OUT_COMPACT, MARG_OUT_BS = MARG_OUT_AS + 6400,
       MARG_OUT_STRIDE = MARG_OUT_BS + 80 };
// per-workgroup scratch in HBM (L2-resident): Z = diag(sqrt(lam^+)) V' Amr, its right-hand side, and the eigenvector matrix of the
// Jacobi safety net for A' (the LDS holds one n x n matrix, not two)
enum { MARG_SCR_Z = 0, MARG_SCR_PR = MARG_MAX_M * MARG_MAX_N, MARG_SCR_V = MARG_SCR_PR + 256, MARG_SCR_STRIDE = MARG_SCR_V + (MARG_MAX_N + 1) * (MARG_MAX_N + 2) };

struct MargHdr {
    int nblk, pos, m, n, nx;
    int n_imu, n_proj, prior_n, prior_nblk, prior_xsize;
    int o_blk;     // nblk x 5: gsize, goff, mloc (-1 constant), kind, xsrc (offset in the solve state, -1 none)
    int o_imu;     // n_imu x 4
    int o_proj;    // n_proj x 4
    int o_prior;   // prior_nblk x 4: blk, idx, gsize, x0 offset
    int o_pcol;    // prior_n: mloc index of every J0 column (-1 constant)
    int d_x, d_imu, d_proj, d_prior, d_misc;
    long long ibase, dbase;
    int prior_k0, pad_k0;  // leading zero rows of the prior's J0 | r0 that are not stored (WinHdr::prior_k0, tcv_packed.h)
    long long prior_abs;   // >= 0: J0 | r0 | x0 of the prior are read from the solve batch's data pool at this offset (the marginalised factor
                           // set holds the same prior object as the solve problem: no second copy is packed or uploaded)
    int solve_window;
    long long imu_abs;     // >= 0: the (single) IMU factor's 287 constants are read from the solve batch's data pool at this offset (the
                           // factor is one of the solve problem's: no second copy is packed, uploaded or spliced)
    int block_mode;   // 1: the marginalised inverse depths (1 x 1 blocks) are eliminated by scalar pivots while the factors are
                      // accumulated, only the frame part of the dropped set (m) goes through the eigen pseudo-inverse
    int o_plast;      // block mode: n_proj flags, 1 = last factor of its landmark (factors sorted by landmark)
    // block mode, chunked path (proj_disjoint, no Td): the factors come in chunks of whole landmarks (<= 64 factors, <= MARG_CB_LM eliminated
    // landmarks); per chunk the landmarks' couplings C (landmark x camera column), diagonals and gradients are accumulated next to the
    // camera-camera J'J, and A -= C diag(1/hll) C', b -= C diag(1/hll) gl is ONE rank-16 update on the matrix cores
    int n_pchunk, o_pchunk;   // n_pchunk x 4: first factor, factors, eliminated landmarks, offset of the chunk's group table behind o_pgrp
    int o_plm;                // n_proj: index of the factor's landmark among the chunk's eliminated landmarks (-1: its landmark is a regular column)
    int o_pgrp, pad_pgrp;     // per chunk: [frames nfr | landmark runs nlg | 1 if every factor shares its first pose and its extrinsic block | length |
                              //  (first, count) x nfr into the list at the end | (first factor, count) x nlg | the chunk's factors grouped by their
                              //  second pose, factor order inside a group]: the task decomposition of the accumulation (marg_kernel)
    int cb_off, cb_stride;    // LDS offset (doubles) and row stride of C: [MARG_CB_LM x cb_stride | hll MARG_CB_LM | gl MARG_CB_LM]; cb_off < 0: old path
    int td_blk;       // >= 0: the point factors are ProjectionTdFactors on this block (d_proj then holds 14 doubles per factor)
    int sqrt_src;        // >= 0: index of the (single) IMU factor among the solve problem's IMU factors: its sqrt_info was computed by the solve
    int proj_disjoint;   // 1: no block is the frame-i pose of one point factor and the frame-j pose of another (MARGIN_OLD: every factor is
                         // anchored in the dropped frame), so one thread can own one entry of the 19 x 20 record across all factors of a chunk
};

struct MargArgs {
    const MargHdr *hdr;
    const int *ipool;
    const double *dpool;
    const double *solve_state;   // may be null
    const double *solve_sqrt;    // may be null: per window 225 doubles, the solve's sqrt_info of IMU factor sqrt_src
    const double *solve_dpool;   // the solve batch's data pool (MargHdr::prior_abs)
    const void *solve_win;       // its window headers (WinHdr): prior_k0 of a prior whose zero-row count was only known on the device (MargHdr::prior_k0 < 0)
    double *out;                 // per window MARG_OUT_STRIDE
    int *out_status;             // per window: 0 ok
    double *scratch;             // per workgroup MARG_SCR_STRIDE
    int nwin, state_stride, use_solved_state;
    int eig_mm;                  // 1: Amm^+ through the eigen-decomposition for every window (TCV_MARG_EIG_MM=1: A/B checks)
    int eig_flags;               // developer A/B switches of the eigen-solver of A' (TCV_MARG_EIG_FLAGS): 1 = round 2's eigenvalue search (every eigenvalue, 4- / 7-section), 2 = reflector-by-reflector back-transformation on the VALU
};

// the 64 diagnostic doubles behind x in the result block (written by marg_kernel and its eigen-solvers, read by the TCV_DEBUG dump of
// tcv_marg_get_prior); the cycle counters are filled by the profiling build only
enum {
    MARG_DIAG = MARG_OUT_X + MARG_MAX_X,
    MARG_DIAG_SWEEPS_MM = MARG_DIAG,            // Jacobi sweeps of Amm (0: Cholesky route), of the safety net of A' (+ 100; 0: not needed)
    MARG_DIAG_SWEEPS_RR = MARG_DIAG + 1,
    MARG_DIAG_PHASE = MARG_DIAG + 2,            // 12 cycle counters of the kernel's phases (MARG_MARK; 9 .. 11: jacobi_eig, or the Cholesky route of Amm)
    MARG_DIAG_EIG_CHECK = MARG_DIAG + 14,       // sym_eig_tridiag's self-check: dev, sum(lam), trace, |T|, lam_min, lam_max
    MARG_DIAG_EIG_PHASE = MARG_DIAG + 22,       // 6 cycle counters of its phases (EMARK)
    MARG_DIAG_TRIDIAG_STEP = MARG_DIAG + 28,    // 6 cycle counters inside the tridiagonalisation step (SMARK)
    MARG_DIAG_AMM_TRACE = MARG_DIAG + 40,       // trace(Amm^-1), and of the unit-diagonal scaling
    MARG_DIAG_PROJ_SUB = MARG_DIAG + 44,        // 4 cycle counters of the chunked block path (MARG_SUB)
};

}  // namespace tcv

// sets the dynamic-LDS size and launches marg_kernel's 256-thread (nt == MARG_NT_PAIR) or 512-thread instance; TCV_OK or TCV_ERR_HIP
int tcv_launch_marg(const tcv::MargArgs *args, int grid, int nt, size_t lds_bytes, hipStream_t st);
