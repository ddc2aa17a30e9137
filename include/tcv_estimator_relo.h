/* tcv_estimator_relo.h -- relocalisation in the native estimator: the loop-closure frame of the pose graph as one more pose block of the
 * next window, and the drift correction that window's solution gives.  Part of include/tcv_estimator.h, which includes this file:
 * include that one.
 *
 * Reference: Estimator::setReloFrame (estimator.cpp:2261-2279, called from estimator_node.cpp:352-377 whenever the pose graph reports a
 * loop), relo_Pose and its ProjectionFactors in the window (:1854-1886), the tail of double2vector (:1606-1624) and what the node publishes
 * of it (utility/visualization.cpp:194-195 the corrected pose, :463-473 relo_relative_t / _q / _yaw).  clearState resets the drift
 * (:185-188).  The solver side is tcv_problem_set_relocalization / tcv_relo_result (include/tcv.h).
 * Out of scope: the pose graph that produces the matches, and applying the correction to the published trajectory -- the caller does
 * drift_correct_r * P + drift_correct_t, as visualization.cpp does.
 */
#ifndef TCV_ESTIMATOR_RELO_H
#define TCV_ESTIMATOR_RELO_H
#include "tcv_estimator.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Frame identity.  The ABI carries no time stamps, so a frame is named by its serial: the number of successful begin_frame calls of this
 * estimator before its own, counted from 0 since create or reset (it stands in for Headers[i].stamp of :2271).  *next_serial = the serial
 * the next begin_frame gets; window_serials[WINDOW_SIZE + 1] = the serial of the frame in every slot, -1 for a slot that holds none;
 * *n_slots = slots that hold a frame (between frames: 0 .. WINDOW_SIZE, the newest slot is empty; between a begin_frame that reported
 * ready and its finish_frame: WINDOW_SIZE + 1).  Any of the three pointers may be NULL. */
int tcv_estimator_frame_serial(const tcv_estimator *e, int *next_serial, int *window_serials, int *n_slots);

/* Estimator::setReloFrame.  Called between frames (estimator_node.cpp:376: behind the previous frame's finish_frame, before the next
 * begin_frame); between a begin_frame that reported ready and its finish_frame it returns TCV_ERR_INVALID.
 *   frame_serial: the window frame the loop-closure frame was matched with; slots 0 .. WINDOW_SIZE - 1 are searched (:2269: not the newest slot).
 *                 Not there: TCV_OK, *accepted = 0, nothing changes (a request made earlier stays) -- the reference ignores it silently, too.
 *   frame_index:  relo_frame_index, the pose graph's index of the loop-closure frame: handed back with the result.
 *   match_points: n_match x 3 = x, y (normalised plane of the loop-closure frame), feature id; copied.  STRICTLY ASCENDING in id, otherwise
 *                 TCV_ERR_INVALID: :1870-1874 walks the list once, in the order of the feature list.  The reference's walk has no end
 *                 check (it reads past the last match when a later feature has a larger id); this one stops at the end of the list.
 *   prev_relo_t / prev_relo_r (row-major): pose of the loop-closure frame in the pose graph's drift-free frame.
 * Found: *accepted = 1; the request replaces a pending one and is consumed by the next optimised window of this estimator, in which
 * relo_Pose -- started from the slot's CURRENT pose as vector2double writes it -- is one more pose block and every feature of the window
 * (used_num >= 2, start_frame < WINDOW_SIZE - 2) with start_frame <= the slot and its id in match_points gets one more
 * ProjectionFactor(first observation, (x, y, 1)) on (para_Pose[start_frame], relo_Pose, para_Ex_Pose[0], para_Feature[feature_index]) with
 * the window's sqrt_info and CauchyLoss (:1854-1886).  The marginalisation problems never see any of it (:1911-2113).
 * Deviations, both documented in DESIGN.md section 8: the reference copies para_Pose[i] (:2276), which at that moment still holds the
 * PREVIOUS window's array (one slide behind) -- a start value of a free block only; and a request none of whose matches lands on a feature
 * of the window is consumed without a relo_Pose block (the reference would add a block no residual touches).
 * With ESTIMATE_TD on (tcv_estimator_set_time_offset): TCV_ERR_INVALID -- the reference would mix a plain ProjectionFactor into a window
 * of ProjectionTdFactors, which the solver's problem model excludes (tcv.h: a problem holds either).
 * tcv_estimator_reset drops a pending request and resets the drift to identity / zero (:185-188). */
int tcv_estimator_set_relo_frame(tcv_estimator *e, int frame_serial, int frame_index, int n_match, const double *match_points,
                                 const double prev_relo_t[3], const double prev_relo_r[9], int *accepted);

/* What the last APPLIED relocalisation window left (double2vector :1606-1620): valid = 0 before the first one (drift_correct_r identity,
 * everything else zero); the drift pair persists until the next relocalisation, as in the reference.  A relocalisation window that is
 * not applied (its solve failed) consumes the request and leaves this record alone.  Matrices row-major, quaternion x y z w, yaw in degrees. */
typedef struct tcv_estimator_relo {
    int valid, frame_index, frame_serial, pad_;
    double drift_correct_r[9], drift_correct_t[3];
    double relo_relative_t[3], relo_relative_q[4], relo_relative_yaw;
    double relo_r[9], relo_t[3];
} tcv_estimator_relo;
int tcv_estimator_get_relocalization(const tcv_estimator *e, tcv_estimator_relo *out);

/* The relocalisation part of the window tap (tcv_estimator_set_window_tap; tcv_window_snapshot keeps its layout): has_relo = 0 for a
 * window without one (everything else zero / NULL).  local_index = relo_frame_local_index, frame_index / frame_serial as given;
 * relo_pose_in / _out = relo_Pose before and after the solve (un-fixed: the reference never writes it back; zeros when the window was not
 * applied); the n_relo factors: relo_frame_i = start_frame, relo_feature = feature_index, relo_pts = n_relo x 6 (pts_i | pts_j);
 * prev_relo_t / _r; result = the window's tcv_relo_result (valid = 0 when the window was not applied).  Same lifetime as the other snapshot arrays. */
typedef struct tcv_window_snapshot_relo {
    int has_relo, local_index, n_relo, frame_index, frame_serial, pad_;
    double relo_pose_in[7], relo_pose_out[7];
    const int *relo_frame_i, *relo_feature;
    const double *relo_pts;
    double prev_relo_t[3], prev_relo_r[9];
    tcv_relo_result result;
} tcv_window_snapshot_relo;
int tcv_estimator_get_window_snapshot_relo(const tcv_estimator *e, tcv_window_snapshot_relo *out);

#ifdef __cplusplus
}
#endif
#endif
