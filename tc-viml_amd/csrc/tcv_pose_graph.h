// Edge maths of the 4-DoF pose graph (reference pose_graph/src/pose_graph.h:89-246), shared by the kernels and the host side of
// tcv_pose_graph.hip: the single-wrap NormalizeAngle, the residual of FourDOFError / FourDOFWeightError with its analytic Jacobians (the
// reference auto-differentiates) and Ceres' corrector for the Huber loss.  Angles are degrees, as in the reference.
#pragma once
#include "tcv_gauge.h"

namespace tcv {

enum { PG_BW = 19, PG_LD = 20 };      // scalar half-bandwidth of the band (4 blocks of 4 + 3) and the row length of its storage

struct PgOpts {      // tcv_pose_graph_options, flattened for the kernels
    int max_it, pad_;
    double huber, weight, yaw_div, ftol, gtol, ptol, radius0, min_rel_dec;
};

// pose_graph.h:89-97 (one wrap only: NOT Utility::normalizeAngle)
TCV_HD double pg_normalize_angle(double a) { return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a); }

// One edge between node i (older) and node j.  x = (yaw, tx, ty, tz); meas = [relative_t 3 | relative_yaw | pitch_i | roll_i]; kind 1: the
// weighted loop edge.  r: 4 residuals; Ji / Jj: 4 x 4 row-major, columns (yaw, tx, ty, tz); both may be NULL.  Returns the cost rho(|r|^2) / 2;
// with `correct` the residual and the Jacobians come back scaled by sqrt(rho') (Ceres' Corrector with alpha = 0: Huber has rho'' <= 0).
TCV_HD double pg_edge(int kind, const double *xi, const double *xj, const double *meas, const PgOpts &o, bool correct, double *r, double *Ji, double *Jj) {
    const double k = TCV_PI / 180.0;
    const double y = xi[0] * k, p = meas[4] * k, ro = meas[5] * k;
    const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(ro), sr = sin(ro);
    // w_R_i (pose_graph.h:118-135) and its derivative by the yaw in degrees
    const double R[9] = {cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, -sp, cp * sr, cp * cr};
    const double dR[6] = {-sy * cp * k, (-cy * cr - sy * sp * sr) * k, (cy * sr - sy * sp * cr) * k, cy * cp * k, (-sy * cr + cy * sp * sr) * k, (sy * sr + cy * sp * cr) * k};
    const double d0 = xj[1] - xi[1], d1 = xj[2] - xi[2], d2 = xj[3] - xi[3];
    const double w = kind ? o.weight : 1.0, wy = kind ? o.weight / o.yaw_div : 1.0;
    double res[4];
    for (int a = 0; a < 3; a++) res[a] = (R[a] * d0 + R[3 + a] * d1 + R[6 + a] * d2 - meas[a]) * w;      // R^T d
    res[3] = pg_normalize_angle(xj[0] - xi[0] - meas[3]) * wy;
    const double s = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3];
    double cost = 0.5 * s, c = 1.0;
    if (kind && o.huber > 0.0 && s > o.huber * o.huber) {      // HuberLoss::Evaluate
        const double n = sqrt(s);
        cost = 0.5 * (2.0 * o.huber * n - o.huber * o.huber);
        c = sqrt(fmax(2.2250738585072014e-308, o.huber / n));
    }
    if (!correct) c = 1.0;
    if (r) for (int a = 0; a < 4; a++) r[a] = c * res[a];
    if (Ji) {
        for (int a = 0; a < 3; a++) {
            Ji[4 * a] = c * w * (dR[a] * d0 + dR[3 + a] * d1);
            for (int b = 0; b < 3; b++) { Ji[4 * a + 1 + b] = -c * w * R[3 * b + a]; Jj[4 * a + 1 + b] = c * w * R[3 * b + a]; }
            Jj[4 * a] = 0.0;
        }
        Ji[12] = -c * wy; Jj[12] = c * wy;
        for (int b = 1; b < 4; b++) { Ji[12 + b] = 0.0; Jj[12 + b] = 0.0; }
    }
    return cost;
}

}  // namespace tcv
