/* Bundle adjustment of the initial structure from motion, batched on the device: the vision-only full BA at the end of GlobalSFM::construct
 * of the reference (vins_estimator/src/initial/initial_sfm.cpp:232-303, the cost functor initial_sfm.h:25-54) as one device batch of
 * independent problems.  It refines the up-to-scale camera poses and points that tcv_vi_align (include/tcv_vi_alignment.h) takes.
 *
 * What makes the initial values (relativePose, the PnP and triangulation chain) and the per-frame solvePnP behind it stay with the
 * caller.  There is no CPU path.
 *
 * Per problem, in the convention Ceres sees at :236-272: F camera poses (camera from world: p = R(q) X + t, q in w x y z order) and the
 * 3-D points with state == true, each with its observations in normalised image coordinates.  c_rotation[l], c_translation[l] and
 * c_translation[F - 1] are constant (:248-255).  Residual ReprojectionError3D without a loss; the rotations move by
 * ceres::QuaternionParameterization (Plus(q, d) = [cos|d|, sin|d| / |d| d] * q, nothing renormalised).  Ceres' Levenberg-Marquardt loop
 * with an exact step: every point is eliminated into the reduced camera system, which is factorised densely.  FP64,
 * fixed summation orders: the same bits from run to run and whether a problem is solved alone or at any position of any batch.
 *
 * Deviations from the reference.  Solver::Options::max_solver_time_in_seconds = 0.2 (:277) is a wall clock of the host CPU and is not
 * reproduced: max_num_iterations is the only cap.  DENSE_SCHUR's own elimination ordering is not reproduced either (the step is exact
 * either way, only rounding differs).
 *
 * Limits (TCV_ERR_UNSUPPORTED before anything is launched): TCV_SFM_BA_MAX_FRAMES frames and TCV_SFM_BA_MAX_POINTS points per problem,
 * TCV_SFM_BA_MAX_BATCH problems per call (and 2 GiB of device scratch per call).  Valid C99 and C++14. */
#ifndef TCV_SFM_BA_H
#define TCV_SFM_BA_H
#include "tcv.h" /* the error codes */

#ifdef __cplusplus
extern "C" {
#endif

#define TCV_SFM_BA_MAX_FRAMES 15   /* the reference uses WINDOW_SIZE + 1 = 11 */
#define TCV_SFM_BA_MAX_POINTS 1024 /* the solve kernel's landmark limit */
#define TCV_SFM_BA_MAX_BATCH 4096
#define TCV_SFM_BA_MAX_TRACE 64    /* iteration 0 + 50 iterations fit */

typedef struct tcv_sfm_ba_desc {
    int n_frames;               /* F >= 2                                                                            */
    int l;                      /* the reference frame: 0 <= l < F                                                   */
    const double *c_rotation;   /* F x 4, (w, x, y, z), camera from world; not the zero quaternion                   */
    const double *c_translation; /* F x 3                                                                            */
    int n_points;               /* >= 1                                                                              */
    const double *position;     /* n_points x 3                                                                      */
    const int *obs_first, *obs_count; /* per point: its observations are obs_first[p] .. obs_first[p] + obs_count[p] - 1, at least 2 */
    int n_obs;                  /* length of obs_frame, obs_uv / 2                                                   */
    const int *obs_frame;       /* the frame of every observation; a point sees a frame once at most                 */
    const double *obs_uv;       /* n_obs x 2, normalised image coordinates                                           */
} tcv_sfm_ba_desc;

/* named after Ceres' Solver::Options; the defaults reproduce the reference (:274-277 and Ceres' own defaults) */
typedef struct tcv_sfm_ba_options {
    int max_num_iterations;             /* 50                                                                       */
    int max_num_consecutive_invalid_steps; /* 5                                                                     */
    double function_tolerance;          /* 1e-6                                                                     */
    double gradient_tolerance;          /* 1e-10                                                                    */
    double parameter_tolerance;         /* 1e-8                                                                     */
    double initial_trust_region_radius; /* 1e4                                                                      */
    double min_relative_decrease;       /* 1e-3                                                                     */
    double accept_cost;                 /* 5e-3 (:281)                                                              */
} tcv_sfm_ba_options;
void tcv_sfm_ba_options_default(tcv_sfm_ba_options *o);

typedef struct tcv_sfm_ba_summary {
    int iterations;  /* records: iteration 0 + accepted + rejected + invalid steps (may exceed TCV_SFM_BA_MAX_TRACE: counted, not stored); 0: FAILURE at entry */
    int termination; /* as tcv_solver_summary::termination: 0 NO_CONVERGENCE 1 gradient 2 parameter 3 function 4 radius 5 FAILURE */
    int accepted;    /* termination is a CONVERGENCE || final_cost < accept_cost (:281)                                          */
    int num_camera_unknowns, num_points, num_observations;
    double initial_cost, final_cost;
    /* the first TCV_SFM_BA_MAX_TRACE records */
    double cost[TCV_SFM_BA_MAX_TRACE], cost_candidate[TCV_SFM_BA_MAX_TRACE], rho[TCV_SFM_BA_MAX_TRACE], radius[TCV_SFM_BA_MAX_TRACE];
    int step[TCV_SFM_BA_MAX_TRACE]; /* 1 accepted (and iteration 0), 0 rejected (and the record of a tolerance stop), -1 invalid */
} tcv_sfm_ba_summary;

typedef struct tcv_sfm_ba_result {
    double *c_rotation;    /* F x 4, the refined camera-frame poses                                                  */
    double *c_translation; /* F x 3                                                                                  */
    double *position;      /* n_points x 3                                                                           */
    /* optional (either may be NULL): the world-frame pair of :290-303 for the PnP stage, computed from the three arrays above in this
     * order: n = ((w w + x x) + y y) + z z, q[i] = (w, -x, -y, -z) / n; u = 2 (v x c), T[i] = -(c + w u + v x u), v the vector part of q[i],
     * c = c_translation[i] (Eigen's inverse() and operator*) */
    double *q;             /* F x 4, (w, x, y, z)                                                                    */
    double *T;             /* F x 3                                                                                  */
    tcv_sfm_ba_summary summary;
} tcv_sfm_ba_result;

/* All n problems as ONE device batch: one upload, one kernel on `hip_stream` (NULL, a hipStream_t or TCV_STREAM_THREAD), one download;
 * returns when the results are on the host.  options NULL: the defaults.  A problem that fails (a factorisation that keeps failing, a
 * non-finite residual at entry) reports termination 5 in its own summary and comes back with its last accepted state (never NaN); it
 * does not fail the call and its neighbours are untouched.
 * TCV_ERR_INVALID (before the device is touched): NULL arrays, F < 2, l out of range, n_points < 1, a point with fewer than 2
 * observations, an observation range or a frame index out of range, a point that sees a frame twice, non-finite input, a zero quaternion.
 * TCV_ERR_NO_DEVICE without a device. */
int tcv_sfm_ba(int n, const tcv_sfm_ba_desc *descs, const tcv_sfm_ba_options *options, tcv_sfm_ba_result *results, void *hip_stream);

/* Residual, Jacobians and cost of n independent observations on the device (the counterpart of tcv_pose_graph_eval_edges).  Per
 * observation: rotation 4 (w x y z, any norm but zero), translation 3, point 3, uv 2.  Out: residual 2, jacobian 18 = d r / d (rotation
 * tangent 3 | translation 3 | point 3) 2 x 9 row-major, cost (|r|^2 / 2).  A point on the camera's plane z = 0 gives non-finite values. */
int tcv_sfm_ba_eval_observations(int n, const double *rotation, const double *translation, const double *point, const double *uv,
                                 double *residual, double *jacobian, double *cost);

/* Host only.  out[8] = { camera tangent dimension, points, observations, LDS bytes of the problem's workgroup, scratch bytes on the
 * device, row length of the reduced camera system in LDS, points per Schur chunk, 0 } */
int tcv_sfm_ba_plan_stats(const tcv_sfm_ba_desc *desc, long long *out);

/* The calling thread's last tcv_sfm_ba: out[4] = host packing, upload, kernel, download in milliseconds (the three device figures from
 * events on the call's stream). */
int tcv_sfm_ba_last_timing(double *out);

#ifdef __cplusplus
}
#endif
#endif
