/* Marginal covariance of window states, batched on the device: the counterpart of ceres::Covariance (Compute +
 * GetCovarianceBlockInTangentSpace) for every window of a resident batch (include/tcv.h tcv_batch_create).
 *
 * Per window, at the evaluation point: H = J'J in tangent space with the loss-corrected Jacobians and the prior's rows, the landmarks
 * eliminated (S = H_cc - sum_l h_l h_l' / H_ll), Cholesky of S, and the requested blocks of S^-1 -- the marginal covariance of the
 * camera-side states.  FP64, every sum in a fixed order that depends on the window alone: the same bits from run to run and whether a
 * window is alone or inside any batch; block (i, j) is the exact transpose of block (j, i), diagonal blocks are exactly symmetric.
 * The call changes nothing the solve, the gauge fix, the marginalisation or the evaluation read or write.  There is no CPU path.
 *
 * Limits: camera-side blocks only -- a landmark (inverse depth) block needs 1 / H_ll + w'Cw over every pose that sees the landmark and is
 * refused with TCV_ERR_UNSUPPORTED; blocks come back in TANGENT space (a pose is 6 wide: translation, rotation), the ambient form is
 * left to the caller (tcvshim::Covariance::GetCovarianceBlock, include/tcv_ceres_shim.hpp); at most TCV_COVARIANCE_MAX_DIM tangent
 * dimensions on the camera side; a rank-deficient window is reported, never pseudo-inverted.  The native estimator (tcv_estimator.h) does
 * not call this yet.  Valid C99 and C++14. */
#ifndef TCV_COVARIANCE_H
#define TCV_COVARIANCE_H
#include "tcv.h" /* the error codes, tcv_batch, tcv_problem, TCV_STREAM_THREAD */

#ifdef __cplusplus
extern "C" {
#endif

#define TCV_COVARIANCE_MAX_DIM 184    /* camera-side tangent dimensions of one window                       */
#define TCV_COVARIANCE_MAX_BLOCKS 512 /* requested blocks per call                                          */
/* default of tcv_covariance_options::min_relative_pivot: the geometric middle (2.7e-13) between the smallest relative pivot of the
 * well-posed test population (3.6e-11) and the largest |pivot| at which windows without a gauge fail (2.1e-15, rounding noise); the
 * figures: tests/test_covariance_cpu.py, profiles/covariance.txt, DESIGN.md section 8 */
#define TCV_COVARIANCE_MIN_RELATIVE_PIVOT 3e-13

typedef struct tcv_covariance_options {
    int at_solution;           /* 0: the uploaded initial states; 1: the states the last solve left (as tcv_evaluate_options::at) */
    int apply_loss_function;   /* 1 (ceres::Covariance::Options::apply_loss_function)                                              */
    double min_relative_pivot; /* rank gate: pivot k of the Cholesky factorisation fails when L_kk^2 <= min_relative_pivot * S_kk  */
} tcv_covariance_options;
void tcv_covariance_options_default(tcv_covariance_options *o);

typedef enum {
    TCV_COV_POSE = 0,       /* para_Pose[index]                                    6 x 6 */
    TCV_COV_SPEED_BIAS = 1, /* para_SpeedBias[index]                               9 x 9 */
    TCV_COV_EXTRINSIC = 2,  /* para_Ex_Pose[0]: index 0                            6 x 6 */
    TCV_COV_TD = 3,         /* para_Td[0]: index 0                                 1 x 1 */
    TCV_COV_RELO_POSE = 4,  /* relo_Pose (tcv_problem_set_relocalization): index 0 6 x 6 */
    TCV_COV_LANDMARK = 5    /* para_Feature[index]: TCV_ERR_UNSUPPORTED                  */
} tcv_covariance_kind;

/* One requested block cov(block i, block j).  A frame index counts from the oldest frame of the window (tcv_problem_set_frames /
 * tcv_problem_from_window); a negative one counts from the newest, -1 is the newest frame. */
typedef struct tcv_covariance_block {
    int kind_i, index_i;
    int kind_j, index_j;
} tcv_covariance_block;

/* per-window status of the last tcv_batch_compute_covariance */
#define TCV_COVARIANCE_OK 0
#define TCV_COVARIANCE_RANK_DEFICIENT 1 /* a pivot at or below the gate: every requested block of the window is zero (never NaN) */
#define TCV_COVARIANCE_NON_FINITE 2     /* NaN / Inf met in the factorisation: every requested block of the window is zero         */

/* The same `n_blocks` requests for every window of the batch, asynchronous on `hip_stream` like tcv_batch_evaluate (NULL, a hipStream_t
 * or TCV_STREAM_THREAD).  A rank-deficient window does not fail the call: it returns TCV_OK and says so in its status.  A call with another
 * request list than the previous one on this batch first waits for the batch's work in flight (the result buffers are replaced).
 * Before anything is launched:
 *   TCV_ERR_INVALID      NULL batch / options / blocks, n_blocks outside 1 .. TCV_COVARIANCE_MAX_BLOCKS, an unknown kind, an index out of
 *                        range, at_solution before a solve, a negative or non-finite min_relative_pivot -- and a window that LACKS a
 *                        requested block (td in a window without para_Td, a relocalisation pose in a window without one, the extrinsic
 *                        in a window without point factors, a frame table that was never set): that fails the whole call, there is no
 *                        per-window status for it
 *   TCV_ERR_UNSUPPORTED  a landmark block; a camera side wider than TCV_COVARIANCE_MAX_DIM
 * A block that is constant in a window (the extrinsic with estimate_extrinsic = 0) comes back as zeros, as Ceres does. */
int tcv_batch_compute_covariance(tcv_batch *b, const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks, void *hip_stream);

/* The k-th requested block of one window, row-major rows x cols, in tangent space (waits for the computation).  out holds cap doubles
 * (too few: TCV_ERR_INVALID); rows / cols may be NULL. */
int tcv_batch_get_covariance(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols);
/* The k-th requested block of EVERY window in one device round trip: out = n x rows x cols, n the batch size */
int tcv_batch_get_covariance_all(tcv_batch *b, int k, double *out, int cap, int *rows, int *cols);
/* per-window status (TCV_COVARIANCE_*), n = the batch size */
int tcv_batch_covariance_status(tcv_batch *b, int *out, int n);

/* One problem at the caller's current block values: a one-window batch, computed and read back.  out[k] holds rows x cols doubles of
 * request k (the sizes of the kinds above); *status the window's TCV_COVARIANCE_* (may be NULL).  The requests are validated first
 * (TCV_ERR_INVALID / TCV_ERR_UNSUPPORTED as above), then the device is asked for: TCV_ERR_NO_DEVICE without one, the caller's memory
 * untouched. */
int tcv_problem_compute_covariance(tcv_problem *p, const tcv_covariance_options *o, const tcv_covariance_block *blocks, int n_blocks,
                                   double *const *out, int *status);

/* Host only: the rank gate's decision for one pivot (what the kernel applies): d = L_kk^2, s = S_kk.  Returns a TCV_COVARIANCE_* status. */
int tcv_covariance_pivot_status(double d, double s, double min_relative_pivot);

#ifdef __cplusplus
}
#endif
#endif
