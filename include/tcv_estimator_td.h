/* tcv_estimator_td.h -- ESTIMATE_TD in the native estimator: the online camera-IMU time offset (with the rolling-shutter terms TR / ROW).
 * Part of include/tcv_estimator.h, which includes this file: include that one.
 *
 * Reference: Estimator::td / para_Td (estimator.cpp:51, :170, :1533-1534, :1601-1602), ProjectionTdFactor in the window and in MARGIN_OLD
 * (:1757-1763, :1970-1979), para_Td mapped onto itself by both marginalisation flavours (:2035-2038, :2101-2104), the per-observation
 * velocity / uv / cur_td of FeaturePerFrame (feature_manager.h:135-149, feature_manager.cpp:215, :271).  compensatedParallax2, triangulate,
 * removeBackShiftDepth, failure detection and the line association do not look at td in the reference and do not here.
 * The solver side is tcv_window_desc::para_td / proj_td_aux / td_TR / td_ROW (include/tcv.h).
 */
#ifndef TCV_ESTIMATOR_TD_H
#define TCV_ESTIMATOR_TD_H
#include "tcv_estimator.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ESTIMATE_TD.  The globals ESTIMATE_TD, TD, TR, ROW (parameters.cpp:135-138) of this estimator: with estimate_td != 0 every point factor
 * of its windows is a ProjectionTdFactor on the extra block para_Td[0] (estimator.cpp:1703-1707, :1757-1763, :1970-1979), td is
 * optimised with the window (vector2double :1533-1534, double2vector :1601-1602) and para_Td is a kept block of the marginalisation
 * prior (:2035-2038, :2101-2104).  td0 is the value td starts from and returns to on tcv_estimator_reset (`td = TD`, :51, :170).
 * NOTE: the reference's setParameters -- the variant that loads the line map -- overwrites it with 0 right away (`td = TD; td = 0;`,
 * :88-89); a caller that mirrors that path passes td0 = 0.  TR: rolling-shutter read-out time of a frame in seconds (0: global
 * shutter), ROW: image rows; ROW <= 0 is TCV_ERR_INVALID whatever estimate_td says.
 * Allowed only while the window is empty, i.e. after tcv_estimator_create or tcv_estimator_reset and before the first begin_frame;
 * otherwise TCV_ERR_INVALID (tcv_last_error says why).  The setting survives tcv_estimator_reset, like the rest of the configuration.
 * An estimator that never calls this (or calls it with estimate_td = 0) builds the same windows, bit for bit, as before the call existed.
 * Estimators with and without estimate_td may share a lock-step list. */
int tcv_estimator_set_time_offset(tcv_estimator *e, int estimate_td, double td0, double TR, double ROW);
/* The tail of the front end's 7-vector per tracked point (feature_manager.h:138-147: x y z | u v | velocity x y): aux4 = n_points x 4 =
 * u, v (pixels), velocity x, y (normalised plane, per second), in the order of `point_ids` of the NEXT begin_frame of this estimator --
 * tcv_estimator_begin_frame or its record in tcv_estimators_begin_frames -- which consumes it (copied here: aux4 may go after the call).
 * With estimate_td on, a begin_frame with nothing staged, or with a staged count other than its n_points, returns TCV_ERR_INVALID with a
 * message (in the batched call: in that estimator's rc[i]) and leaves the window as it was.  With estimate_td off staged data is dropped unused. */
int tcv_estimator_stage_point_aux(tcv_estimator *e, int n_points, const double *aux4);
/* Estimator::td after the last applied window (td0 before the first; a window that was not applied leaves it alone).  What the
 * reference does with it outside the estimator stays the caller's job: cutting the IMU samples of a frame at img_t + td and
 * interpolating the last one (estimator_node.cpp:143-166, :311-340). */
int tcv_estimator_get_time_offset(const tcv_estimator *e, double *td);

/* The ESTIMATE_TD part of the same snapshot (the struct above keeps its layout; with estimate_td on its prior_block_kind may hold 3 =
 * para_Td): para_Td[0] before and after the solve (td_out 0 when the window failed), the globals, and proj_td_aux = n_proj x 8 in
 * exactly the layout of tcv_window_desc::proj_td_aux (NULL with estimate_td off or n_proj = 0).  Same lifetime as the arrays above. */
typedef struct tcv_window_snapshot_td {
    int estimate_td, n_proj;
    double td_in, td_out, TR, ROW;
    const double *proj_td_aux;
} tcv_window_snapshot_td;
int tcv_estimator_get_window_snapshot_td(const tcv_estimator *e, tcv_window_snapshot_td *out);

#ifdef __cplusplus
}
#endif
#endif
