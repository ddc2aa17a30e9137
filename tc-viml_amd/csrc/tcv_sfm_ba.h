// Layouts and observation maths shared by the bundle-adjustment kernels (tcv_sfm_ba.hip) and their host half (tcv_sfm_ba_host.cpp):
// include/tcv_sfm_ba.h, the full BA of GlobalSFM::construct (reference initial_sfm.cpp:232-303, ReprojectionError3D initial_sfm.h:25-54).
#pragma once
#include <stddef.h>

#include "tcv_math.h"

namespace tcv {

enum {
    BA_THREADS = 256,
    BA_TILE = 4,          // a thread owns one BA_TILE x BA_TILE tile of the reduced camera system's lower triangle
    BA_CHUNK = 16,        // points per staged chunk of the Schur update: 3 BA_CHUNK rows of Y in LDS
    BA_MAX_NC = 84,       // camera tangent dimension at TCV_SFM_BA_MAX_FRAMES = 15 with l = F - 1: 6 F - 6
    BA_MAX_NCP = 88,      // row length: nc + 1 (the right-hand side rides as one more row / column) rounded up to BA_TILE
    BA_T = 64,            // TCV_SFM_BA_MAX_TRACE
    BA_REC = 38,          // per-observation record in scratch: J_camera 2 x 6 | r 2 | J_point 2 x 3 | Y 6 x 3
    BA_PT = 9,            // per-point record in scratch: L of the damped H_pp (00 10 11 20 21 22) | y = L^-1 g_p
    BA_HC = 27,           // per frame in LDS: lower triangle of its 6 x 6 block of J^T J (21) | its 6 entries of J^T r
    BA_SUM = 4 + 5 * BA_T, // summary record: initial_cost, final_cost, records, termination | cost, cost_candidate, rho, radius, step: BA_T each
    BA_OBS_IN = 12,       // tcv_sfm_ba_eval_observations: rotation 4 | translation 3 | point 3 | uv 2
    BA_OBS_OUT = 21,      // residual 2 | jacobian 18 | cost
};
static_assert((BA_MAX_NCP / BA_TILE) * (BA_MAX_NCP / BA_TILE + 1) / 2 <= BA_THREADS, "one lower tile per thread");
static_assert(BA_MAX_NCP % BA_TILE == 0 && BA_MAX_NCP >= BA_MAX_NC + 1, "the right-hand side fits");

// One problem of a batch; the offsets count ints / doubles from the start of their pools.
//   ints:    obs_frame NO | obs_point NO | point_first P + 1 | frame_ptr F + 1 | frame_obs NO | coff 2 F | colinfo nc
//            (observations in point order; frame_obs: the observations of every frame, ascending; coff[2 f], coff[2 f + 1]: first column of
//            frame f's rotation / translation, -1 constant; colinfo[j] = 6 f + k of camera column j)
//   doubles: c_rotation 4 F | c_translation 3 F | position 3 P | uv 2 NO          (the first 7 F + 3 P are the state vector x)
//   out:     x 7 F + 3 P | summary BA_SUM
struct BaHdr {
    int n_frames, n_points, n_obs, nc;
    long long o_int, o_dbl, o_scr, o_out;
};
inline int ba_ncp(int nc) { return (nc + 1 + BA_TILE - 1) / BA_TILE * BA_TILE; }
inline long long ba_nx(int F, int P) { return 7LL * F + 3LL * P; }
// scratch of one problem, doubles: x | candidate | scale | delta | observation records | point records
inline long long ba_scratch_doubles(int F, int P, int NO, int nc) { return 2 * ba_nx(F, P) + 2 * (nc + 3LL * P) + (long long)BA_REC * NO + (long long)BA_PT * P; }
// dynamic LDS of a workgroup whose problems have at most nc camera unknowns and F frames, doubles:
// reduction 256 | S ncp^2 | chunk 3 BA_CHUNK ncp | Hc 27 F | dinv ncp | ys ncp.  F = 11: 64.6 KB
inline size_t ba_lds_doubles(int nc, int F) {
    const size_t ncp = (size_t)ba_ncp(nc);
    return BA_THREADS + ncp * ncp + 3 * BA_CHUNK * ncp + (size_t)BA_HC * F + 2 * ncp;
}

struct BaOpts {      // tcv_sfm_ba_options, flattened for the kernel
    int max_it, max_invalid;
    double ftol, gtol, ptol, radius0, min_rel_dec;
};

// ReprojectionError3D with its analytic Jacobians in the tangent space of ceres::QuaternionParameterization (the reference
// auto-differentiates).  q = (w, x, y, z) of any norm but zero: p = R(q / |q|) X + t, r = (p_x / p_z - u, p_y / p_z - v).
// Jc: 2 x 6 row-major = d r / d (rotation tangent 3 | translation 3): d p / d d = -2 [R X]x (Plus multiplies on the left by a rotation of
// angle 2 |d|; the norm of q cancels between Plus and the normalisation), d p / d t = I.  Jp: 2 x 3 = d r / d X (d p / d X = R).
// Jc and Jp may both be NULL.  Returns |r|^2 / 2.
TCV_HD double ba_observation(const double *q, const double *t, const double *X, const double *uv, double *r, double *Jc, double *Jp) {
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    const double a = R[0] * X[0] + R[1] * X[1] + R[2] * X[2], b = R[3] * X[0] + R[4] * X[1] + R[5] * X[2], c = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
    const double px = a + t[0], py = b + t[1], pz = c + t[2];
    const double iz = 1.0 / pz;
    const double r0 = px * iz - uv[0], r1 = py * iz - uv[1];
    r[0] = r0; r[1] = r1;
    if (Jc) {
        const double P[6] = {iz, 0.0, -px * iz * iz, 0.0, iz, -py * iz * iz};      // d r / d p
        const double M[9] = {0.0, 2.0 * c, -2.0 * b, -2.0 * c, 0.0, 2.0 * a, 2.0 * b, -2.0 * a, 0.0};      // -2 [R X]x
        for (int row = 0; row < 2; row++)
            for (int k = 0; k < 3; k++) {
                Jc[6 * row + k] = P[3 * row] * M[k] + P[3 * row + 1] * M[3 + k] + P[3 * row + 2] * M[6 + k];
                Jc[6 * row + 3 + k] = P[3 * row + k];
                Jp[3 * row + k] = P[3 * row] * R[k] + P[3 * row + 1] * R[3 + k] + P[3 * row + 2] * R[6 + k];
            }
    }
    return 0.5 * (r0 * r0 + r1 * r1);
}

}  // namespace tcv

extern "C" int tcv_launch_sfm_ba(int n, const tcv::BaHdr *hdrs, const int *ipool, const double *dpool, double *scratch, double *out, tcv::BaOpts opts,
                                 size_t lds_bytes, void *stream);
extern "C" int tcv_launch_sfm_ba_observations(int n, const double *in, double *out, void *stream);
