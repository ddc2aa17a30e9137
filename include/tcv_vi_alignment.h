/* Visual-inertial alignment on the device: the inertial half of the reference's initialisation, VisualIMUAlignment
 * (vins_estimator/src/initial/initial_aligment.cpp:3-207: solveGyroscopeBias, LinearAlignment, TangentBasis, RefineGravity) followed by the
 * state change of Estimator::visualInitialAlign (estimator.cpp:1380-1438), for n independent sequences as one device batch.  It turns
 * up-to-scale structure-from-motion poses and the raw IMU stream into what tcv_estimator takes through `truth` for its first frames:
 * metric, gravity-aligned Ps / Rs / Vs, the gyroscope bias, the scale and the gravity vector.
 *
 * Per sequence: the F frames of all_image_frame with ImageFrame::R (body rotation in the SfM frame, Q[i] * RIC^T) and ImageFrame::T (camera
 * position in that frame, up to scale), the IMU samples of the F - 1 intervals between them in the layout of tcv_preintegrate, and the
 * window's key frames as indices into the frames.  FP64, fixed summation orders, no atomics: the same bits from run to run and whether a
 * sequence is aligned alone or inside any batch.  There is no CPU path.
 *
 * Left to the caller:
 *   - the visual half but its bundle adjustment: relativePose, the PnP and triangulation chain of GlobalSFM::construct and the per-frame
 *     solvePnP (estimator.cpp:1235-1356); the full BA at the end of construct is tcv_sfm_ba (include/tcv_sfm_ba.h);
 *   - f_manager.triangulate on the camera poses and `estimated_depth *= s` (estimator.cpp:1389-1400, :1419-1425);
 *   - re-propagating the window's own key-frame-to-key-frame pre_integrations[] with `bg` (estimator.cpp:1403-1406): tcv_preintegrate_device
 *     at (0, bg) does that;
 *   - handing the states to tcv_estimator.
 *
 * Deviations from the reference, all documented in DESIGN.md section 8: the linear systems are solved by an unpivoted Cholesky in natural
 * order behind a rank gate (the reference: Eigen's pivoted LDLT, no gate); Quaterniond::FromTwoVectors of g2R takes the fixed axis
 * (1, 0, 0) in its antiparallel branch (Eigen: an axis from an SVD); TangentBasis takes its special branch for gravity exactly along -z
 * of the SfM frame as well as +z (the reference: +z only; at -z its basis is the zero vector).
 *
 * Limits (TCV_ERR_UNSUPPORTED before anything is launched): TCV_VI_ALIGN_MAX_FRAMES frames per sequence, TCV_VI_ALIGN_MAX_BATCH sequences
 * per call.  Valid C99 and C++14. */
#ifndef TCV_VI_ALIGNMENT_H
#define TCV_VI_ALIGNMENT_H
#include "tcv.h" /* the error codes, tcv_imu_preintegration, TCV_STREAM_THREAD */

#ifdef __cplusplus
extern "C" {
#endif

#define TCV_VI_ALIGN_MAX_FRAMES 128
#define TCV_VI_ALIGN_MAX_BATCH 4096

/* tcv_vi_align_result::status */
#define TCV_VI_ALIGN_OK 0           /* aligned                                                                              */
#define TCV_VI_ALIGN_LINEAR 1       /* LinearAlignment's first test: fabs(|g| - G) > 1 || s < 0 (initial_aligment.cpp:184)  */
#define TCV_VI_ALIGN_REFINED_SCALE 2 /* s < 0 after RefineGravity (:193)                                                     */
#define TCV_VI_ALIGN_RANK 3         /* a linear system failed the rank gate                                                 */
#define TCV_VI_ALIGN_NON_FINITE 4   /* NaN or Inf in a result                                                               */

typedef struct tcv_vi_align_desc {
    int n_frames;            /* F, 2 .. TCV_VI_ALIGN_MAX_FRAMES                                                              */
    const double *R;         /* F x 9 row-major: ImageFrame::R                                                               */
    const double *T;         /* F x 3: ImageFrame::T                                                                         */
    double tic[3];           /* TIC[0]                                                                                       */
    /* the IMU samples of the F - 1 intervals, as tcv_preintegrate takes them: interval i (frame i -> i + 1) owns the rows
     * first[i] .. first[i] + count[i] - 1 of samples7 (dt, acc xyz, gyr xyz), count[i] >= 1                                  */
    const int *first, *count;
    const double *samples7;
    int num_samples;
    const double *acc0_gyr0; /* (F - 1) x 6: acc_0, gyr_0 of every interval                                                  */
    double ba0[3], bg0[3];   /* the biases the frames' pre-integrations were created at                                      */
    double noise[4];         /* ACC_N, GYR_N, ACC_W, GYR_W                                                                   */
    int n_key;               /* 1 .. F                                                                                       */
    const int *key_frame;    /* n_key strictly ascending indices into the frames: the window's Headers                       */
} tcv_vi_align_desc;

typedef struct tcv_vi_align_options {
    double gravity_norm;       /* G.norm(), 9.81007                                                                          */
    double min_relative_pivot; /* rank gate: pivot k of a Cholesky factorisation fails when d_k <= min_relative_pivot * A_kk   */
} tcv_vi_align_options;
void tcv_vi_align_options_default(tcv_vi_align_options *o);

/* The arrays are the caller's: velocity, Ps, Rs, Vs must be set before the call, preint may be NULL.  A sequence whose status is not 0
 * returns zeros in everything after the last quantity that was computed:
 *   status 3 in solveGyroscopeBias: everything zero;         status 3 in LinearAlignment / RefineGravity: delta_bg, bg, preint;
 *   status 1: delta_bg, bg, preint, scale and gravity_c0 as LinearAlignment left them (:180-182);
 *   status 2: delta_bg, bg, preint, scale, gravity_c0 (refined) and velocity;      status 4: delta_bg, bg, preint where they are finite. */
typedef struct tcv_vi_align_result {
    int status;
    double delta_bg[3];     /* solveGyroscopeBias (:26)                                                                      */
    double bg[3];           /* bg0 + delta_bg: Bgs[i] (:29-30)                                                               */
    double scale;           /* s, the /100 applied (:190)                                                                    */
    double gravity_c0[3];   /* the refined g in the SfM frame (:122)                                                         */
    double gravity[3];      /* R0 * g (estimator.cpp:1430)                                                                   */
    double rot_diff[9];     /* R0 row-major (estimator.cpp:1427-1432)                                                        */
    double min_pivot;       /* the smallest relative pivot d_k / A_kk of the sequence's factorisations (what the gate looked at) */
    double *velocity;       /* F x 3, body frame: the first 3 F entries of the refined x                                      */
    /* The window states after estimator.cpp:1380-1438.  Vs[kv] = R_{key_frame[kv]} * x.segment<3>(3 * kv) (:1416): the reference indexes x
     * by kv, NOT by the key frame's own position in all_image_frame, and so does this call.  The two agree when the key frames are the
     * first n_key frames; otherwise take the per-frame values from `velocity`. */
    double *Ps;             /* n_key x 3                                                                                     */
    double *Rs;             /* n_key x 9 row-major                                                                           */
    double *Vs;             /* n_key x 3                                                                                     */
    /* optional: the F - 1 pre-integrations re-propagated at (0, bg), what all_image_frame[..].pre_integration holds after
     * solveGyroscopeBias (:32-36: repropagate(Vector3d::Zero(), Bgs[0]) -- ba really is zero there)                          */
    tcv_imu_preintegration *preint;
} tcv_vi_align_result;

/* All n sequences as ONE device batch on `hip_stream` (NULL, a hipStream_t or TCV_STREAM_THREAD); returns when the results are on the host.
 * options NULL: the defaults.  The steps: tcv_preintegrate's kernel at (ba0, bg0), the gyroscope-bias kernel, tcv_preintegrate's kernel
 * again at (0, bg), the alignment kernel (LinearAlignment, RefineGravity, state change); the pre-integration passes run on the calling
 * thread's own stream, as tcv_preintegrate does.  A sequence that fails reports it in its own status; it never fails the call and its
 * neighbours are untouched.
 * TCV_ERR_INVALID (before the device is touched): NULL arrays, F < 2, an interval without samples or outside samples7, key_frame not
 * strictly ascending or out of range, non-finite numbers, options out of range.  TCV_ERR_UNSUPPORTED: beyond a limit above.
 * TCV_ERR_NO_DEVICE without a device. */
int tcv_vi_align(int n, const tcv_vi_align_desc *descs, const tcv_vi_align_options *options, tcv_vi_align_result *results, void *hip_stream);

/* The calling thread's last tcv_vi_align, milliseconds: out[8] = host packing and unpacking, pre-integration pass 1 (its whole round trip),
 * gyroscope-bias round trip, pre-integration pass 2, alignment round trip, and of the two round trips the kernels alone (events on the
 * call's stream): bias kernel, alignment kernel; out[7] = 0. */
int tcv_vi_align_last_timing(double *out);

#ifdef __cplusplus
}
#endif
#endif
