// Relocalisation tail of Estimator::double2vector() (reference vins_estimator/src/estimator.cpp:1606-1624), on top of the gauge fix maths of
// tcv_gauge.h: what the solved relo_Pose says about the drift of the window (drift_correct_r / _t) and about the pose of the matched frame
// relative to the loop-closure frame (relo_relative_t / _q / _yaw), which the reference publishes (utility/visualization.cpp:194-195, :463-473).
// Angles are degrees, as in utility.h.
#pragma once
#include "tcv_gauge.h"

namespace tcv {

// one record per relocalisation window, all doubles: the layout of tcv_relo_result behind its two ints (include/tcv.h)
enum { RELO_R = 0, RELO_T = 9, RELO_DRIFT_R = 12, RELO_DRIFT_T = 21, RELO_REL_T = 24, RELO_REL_Q = 27, RELO_REL_YAW = 31, RELO_DRIFT_YAW = 32, RELO_REC = 33 };
enum { RELO_PREV = 12 };      // prev_relo_t 3 | prev_relo_r 9 (row-major)

// one entry of a batch's relocalisation table (built by the host at tcv_batch_create): the window, where relo_Pose sits in its state vector
// and the local index of the matched frame (relo_frame_local_index)
struct ReloEntry { int window, relo_off, local_index, pad; };

// Utility::normalizeAngle, utility.h:135-143 (degrees)
TCV_HD double normalize_angle(double a) {
    if (a > 0) return a - 360.0 * floor((a + 180.0) / 360.0);
    return a + 360.0 * floor((-a + 180.0) / 360.0);
}

// estimator.cpp:1606-1620.  R0 / P0: Rs[0] / Ps[0] before the solve; pose0, pose_l, relo_pose: the solved, un-fixed para_Pose[0],
// para_Pose[relo_frame_local_index] and relo_Pose; prev: prev_relo_t | prev_relo_r; rec: RELO_REC doubles
TCV_HD void relo_tail(const M3 &R0, const double *P0, const double *pose0, const double *pose_l, const double *relo_pose, const double *prev, double *rec) {
    const M3 rot = gauge_rot_diff(R0, pose0);
    M3 relo_r, Rl; V3 relo_t, Pl, unused;
    gauge_frame(rot, P0, pose0, relo_pose, nullptr, relo_r, relo_t, unused);      // :1610-1613
    gauge_frame(rot, P0, pose0, pose_l, nullptr, Rl, Pl, unused);                 // Rs / Ps[relo_frame_local_index] of the loop :1565-1571
    double a[3], b[3], c[3];
    r2ypr(m3_load(prev + 3), a); r2ypr(relo_r, b); r2ypr(Rl, c);
    const double drift_yaw = a[0] - b[0];                                         // :1615
    const M3 drift_r = ypr2R(drift_yaw, 0.0, 0.0);                                // :1616
    const V3 drift_t = V3(prev) - drift_r * relo_t;                               // :1617
    const M3 relo_rT = transpose(relo_r);
    const V3 rel_t = relo_rT * (Pl - relo_t);                                     // :1618
    const Quat rel_q = r2q(relo_rT * Rl);                                         // :1619 (a Quaterniond assigned from a matrix)
    for (int k = 0; k < 9; k++) { rec[RELO_R + k] = relo_r.m[k]; rec[RELO_DRIFT_R + k] = drift_r.m[k]; }
    rec[RELO_T] = relo_t.x; rec[RELO_T + 1] = relo_t.y; rec[RELO_T + 2] = relo_t.z;
    rec[RELO_DRIFT_T] = drift_t.x; rec[RELO_DRIFT_T + 1] = drift_t.y; rec[RELO_DRIFT_T + 2] = drift_t.z;
    rec[RELO_REL_T] = rel_t.x; rec[RELO_REL_T + 1] = rel_t.y; rec[RELO_REL_T + 2] = rel_t.z;
    rec[RELO_REL_Q] = rel_q.x; rec[RELO_REL_Q + 1] = rel_q.y; rec[RELO_REL_Q + 2] = rel_q.z; rec[RELO_REL_Q + 3] = rel_q.w;
    rec[RELO_REL_YAW] = normalize_angle(c[0] - b[0]);                             // :1620
    rec[RELO_DRIFT_YAW] = drift_yaw;
}

}  // namespace tcv
