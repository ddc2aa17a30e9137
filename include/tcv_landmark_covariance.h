/* Marginal covariance of the landmarks' inverse depths, batched on the device: the landmark rows of ceres::Covariance that
 * include/tcv_covariance.h leaves out.  Per window, with H = J'J as tcv_batch_compute_covariance builds it (loss-corrected Jacobians,
 * the prior's rows, the uploaded or the solved states), c the camera-side tangent space, l one landmark, C = S^-1 = (L L')^-1,
 * h_l = H_cl and w_l = h_l / H_ll:
 *
 *   var(lambda_l)              = 1 / H_ll + w_l' C w_l = 1 / H_ll + |L^-1 w_l|^2
 *   cov(lambda_l, cam block p) = -w_l' C[:, p]         = -(L^-1 w_l) . (L^-1 e_p)
 *
 * The second term of the variance is no correction: on the project's test windows it is 6e-4 to 12 times the first.  The phase runs
 * behind the factorisation of tcv_covariance.h in the same kernel launch (an instantiation of its own: the plain call's kernel is
 * untouched).  FP64, every sum in twice the working precision and in an order that depends on the window alone: the same bits from run
 * to run and whether a window is alone or inside any batch.  The call changes nothing the solve, the gauge fix, the marginalisation,
 * the evaluation or tcv_batch_compute_covariance read or write: the two calls share a batch, each keeps result buffers of its own, and
 * the getters of either return the bits of its own last call whatever the other did in between.
 *
 * Landmark order: landmark l of a window is the problem's l-th inverse-depth block in the order the problem registered them -- the
 * size-1 blocks that point factors name as their fourth block, by first registration (tcv_problem_add_parameter_block, or the first
 * factor that names the address).  For tcv_problem_from_window, whose factors arrive feature by feature, that is para_feature[l].  The
 * device works in the plan's order; the host maps it back.
 *
 * Three behaviours:
 *   - a cross block that is constant in a window (the extrinsic with estimate_extrinsic = 0) returns zero rows, as Ceres does;
 *   - a rank-deficient or non-finite window returns zeros and says so in its status (TCV_COVARIANCE_*); the call returns TCV_OK;
 *   - a landmark whose H_ll is zero (every point factor's derivative by the inverse depth vanishes) returns 0.0: no information is
 *     reported as 0, never as Inf.  A size-1 block WITHOUT any point factor is not a landmark to this library at all: the packer puts it
 *     on the camera side, where a block without information makes the window rank deficient -- a problem cannot hold a landmark without
 *     a point factor, and tcv_problem_compute_landmark_covariance refuses such an address.
 *
 * Out of scope: the covariance between two DIFFERENT landmarks (it needs w_l' C w_k for every pair); calling any of this from the native
 * estimator (tcv_estimator.h does not); a CPU path (there is none: without a device the calls fail with TCV_ERR_NO_DEVICE).
 * Blocks come back in TANGENT space (a pose is 6 wide).  Valid C99 and C++14. */
#ifndef TCV_LANDMARK_COVARIANCE_H
#define TCV_LANDMARK_COVARIANCE_H
#include "tcv_covariance.h" /* tcv_covariance_options, tcv_covariance_kind, TCV_COVARIANCE_* */

#ifdef __cplusplus
extern "C" {
#endif

#define TCV_LANDMARK_COVARIANCE_MAX_CROSS 16 /* cross blocks per call */

/* One camera-side block whose cross covariance with every landmark is asked for: a tcv_covariance_kind other than TCV_COV_LANDMARK,
 * and its index as in tcv_covariance_block (a negative frame index counts from the newest frame). */
typedef struct tcv_landmark_cross_block {
    int kind, index;
} tcv_landmark_cross_block;

/* The variance of every landmark's inverse depth and its cross covariance with `n_cross` (0 .. TCV_LANDMARK_COVARIANCE_MAX_CROSS)
 * camera-side blocks, for every window of the batch; asynchronous on `hip_stream` like tcv_batch_evaluate (NULL, a hipStream_t or
 * TCV_STREAM_THREAD).  `cross` may be NULL when n_cross is 0.  A call with another cross list than the previous landmark call on this
 * batch first waits for the batch's work in flight.  Before anything is launched:
 *   TCV_ERR_INVALID      NULL batch / options, NULL cross with n_cross > 0, n_cross out of range, a landmark kind or an unknown kind in
 *                        `cross`, an index out of range, a window that lacks a requested block (as tcv_batch_compute_covariance),
 *                        at_solution before a solve, a negative or non-finite min_relative_pivot
 *   TCV_ERR_UNSUPPORTED  a constant inverse depth, a factor that names one block twice, a camera side wider than TCV_COVARIANCE_MAX_DIM
 * These three are the checks of tcv_batch_compute_covariance, reused.  Today the packer meets each of them first, when the batch is created
 * (tcv_batch_create, and so inside tcv_problem_compute_landmark_covariance): it refuses a constant inverse depth and a point factor that
 * names one block twice with TCV_ERR_UNSUPPORTED and messages of its own, and a camera side wider than 183 with TCV_ERR_TOO_LARGE -- so
 * the last of the three cannot be reached through this interface. */
int tcv_batch_compute_landmark_covariance(tcv_batch *b, const tcv_covariance_options *o, const tcv_landmark_cross_block *cross, int n_cross,
                                          void *hip_stream);

/* landmarks of one window (known from the batch alone, before any computation) */
int tcv_batch_landmark_covariance_dims(tcv_batch *b, int window, int *n_landmarks);
/* var(lambda_l) of one window, l in the landmark order above (waits for the computation); out holds cap doubles (too few: TCV_ERR_INVALID) */
int tcv_batch_get_landmark_variances(tcv_batch *b, int window, double *out, int cap, int *n);
/* EVERY window in one device round trip: out = n_windows x stride, stride the batch's largest landmark count, the tail of a row zero */
int tcv_batch_get_landmark_variances_all(tcv_batch *b, double *out, int cap, int *stride);
/* cov(lambda_l, cross block k) of one window, row-major rows x cols: rows the window's landmarks, cols the tangent width of the block */
int tcv_batch_get_landmark_cross(tcv_batch *b, int window, int k, double *out, int cap, int *rows, int *cols);
/* per-window status (TCV_COVARIANCE_*) of the last landmark call, n = the batch size */
int tcv_batch_landmark_covariance_status(tcv_batch *b, int *out, int n);

/* One problem at the caller's current block values: a one-window batch, computed and read back.  The landmarks are named by address, as
 * Ceres names blocks: inv_depth_addresses[i], i < n (n >= 1), each an inverse-depth block of the problem (anything else:
 * TCV_ERR_INVALID).  variances holds n doubles; cross_out[k] (k < n_cross; cross_out may be NULL when n_cross is 0) holds n x cols
 * doubles, row i the landmark of address i; *status the window's TCV_COVARIANCE_* (may be NULL).  Everything is validated first
 * (TCV_ERR_INVALID / TCV_ERR_UNSUPPORTED as above; at_solution = 1 needs a solved batch and is TCV_ERR_INVALID here), then the device is
 * asked for: TCV_ERR_NO_DEVICE without one, the caller's memory untouched. */
int tcv_problem_compute_landmark_covariance(tcv_problem *p, const tcv_covariance_options *o, double *const *inv_depth_addresses, int n,
                                            const tcv_landmark_cross_block *cross, int n_cross, double *variances, double *const *cross_out,
                                            int *status);

#ifdef __cplusplus
}
#endif
#endif
