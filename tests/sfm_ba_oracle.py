"""NumPy restatement of the vision-only full bundle adjustment at the end of GlobalSFM::construct (reference
vins_estimator/src/initial/initial_sfm.cpp:232-303, cost functor ReprojectionError3D initial_sfm.h:25-54): the problem of :236-272 with the
constants of :248-255, the residual with analytic Jacobians in the tangent space of ceres::QuaternionParameterization, Ceres' trust-region
loop with LevenbergMarquardtStrategy, the acceptance test of :281 and the world-frame pair of :290-303.  Test infrastructure: the full dense
Jacobian and numpy.linalg.cholesky of the damped normal matrix for the step (DENSE_SCHUR's elimination is not restated: the step is exact
either way).

Like the rest of the oracles it is UNPINNED against a real Ceres: upstream Ceres 2.x as read, every default it relies
on by name in CERES_DEFAULTS below (the shared ones come from pose_graph_oracle.CERES_DEFAULTS and np_oracle.CERES_DEFAULTS).
Solver::Options::max_solver_time_in_seconds = 0.2 (:277) is a wall clock and is not restated."""
from __future__ import annotations

import numpy as np

import np_oracle as NO
import pose_graph_oracle as PO

CERES_DEFAULTS = dict(
    PO.CERES_DEFAULTS,                    # jacobi_scaling 1 / (1 + norm), min / max_lm_diagonal, the tolerances, the radius rules, 5 invalid steps
    max_num_iterations=50,                # Solver::Options default; :274-277 do not set it
    quaternion_plus="[cos|d|, sin|d| / |d| d] * q; a copy for |d| = 0; nothing renormalised",      # QuaternionParameterization::Plus
    candidate_not_finite="cost = DBL_MAX: a rejected step",                                         # ComputeCandidatePointAndEvaluateCost
    parameter_norms="ambient coordinates of the non-constant blocks",
)
ACCEPT_COST = 5e-3      # :281
DBL_MAX = float(np.finfo(float).max)
TERMINATION_CODE = NO.TERMINATION_CODE
decision_margin = PO.decision_margin


def quat_matrix(q):
    """R(q / |q|) for q = (w, x, y, z), (n, 4) -> (n, 3, 3): QuaternionRotatePoint normalises first"""
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_product(a, b):      # ceres::QuaternionProduct, w x y z
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_plus(q, d):      # ceres::QuaternionParameterization::Plus
    n = float(np.sqrt(d @ d))
    if n > 0.0:
        return quat_product(np.concatenate([[np.cos(n)], np.sin(n) / n * d]), q)
    return q.copy()


def observations(q, t, X, uv, want_jac=True):
    """ReprojectionError3D over n observations: residual (n, 2), J (n, 2, 9) = d r / d (rotation tangent 3 | translation 3 | point 3), cost (n).
    d p / d (rotation tangent) = -2 [R X]x: Plus multiplies on the left by a rotation of angle 2 |d|."""
    q, t, X, uv = (np.asarray(a, float) for a in (q, t, X, uv))
    R = quat_matrix(q)
    RX = np.einsum("nij,nj->ni", R, X)
    p = RX + t
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz = 1.0 / p[:, 2]
        r = np.stack([p[:, 0] * iz - uv[:, 0], p[:, 1] * iz - uv[:, 1]], 1)
        cost = 0.5 * (r * r).sum(1)
        if not want_jac:
            return r, None, cost
        n = len(q)
        P = np.zeros((n, 2, 3))
        P[:, 0, 0] = iz; P[:, 0, 2] = -p[:, 0] * iz * iz; P[:, 1, 1] = iz; P[:, 1, 2] = -p[:, 1] * iz * iz
        M = np.zeros((n, 3, 3))
        a, b, c = RX[:, 0], RX[:, 1], RX[:, 2]
        M[:, 0, 1] = 2 * c; M[:, 0, 2] = -2 * b; M[:, 1, 0] = -2 * c; M[:, 1, 2] = 2 * a; M[:, 2, 0] = 2 * b; M[:, 2, 1] = -2 * a
        J = np.concatenate([P @ M, P, P @ R], 2)
    return r, J, cost


class Problem:
    """the problem of :236-272 over dict(c_rotation (F x 4, w x y z), c_translation (F x 3), l, position (P x 3), observations: per point a list
    of (frame, u, v)).  Columns: per frame its free rotation (3) and translation (3), frames ascending, then 3 per point."""

    def __init__(self, p):
        self.rot = np.asarray(p["c_rotation"], float).reshape(-1, 4)
        self.tr = np.asarray(p["c_translation"], float).reshape(-1, 3)
        self.pos = np.asarray(p["position"], float).reshape(-1, 3)
        self.l = int(p["l"])
        F = self.F = len(self.rot)
        self.P = len(self.pos)
        flat = [(k, o) for k, po in enumerate(p["observations"]) for o in po]
        self.opt = np.array([k for k, _ in flat], int)
        self.ofr = np.array([o[0] for _, o in flat], int)
        self.uv = np.array([[o[1], o[2]] for _, o in flat], float).reshape(-1, 2)
        self.col_rot = -np.ones(F, int); self.col_tr = -np.ones(F, int)
        n = 0
        for f in range(F):
            if f != self.l:                      # :248-251
                self.col_rot[f] = n; n += 3
            if f != self.l and f != F - 1:       # :252-255
                self.col_tr[f] = n; n += 3
        self.nc = n
        self.nu = n + 3 * self.P

    def x0(self):
        return (self.rot.copy(), self.tr.copy(), self.pos.copy())

    def evaluate(self, x, want_jac=True):
        rot, tr, pos = x
        return observations(rot[self.ofr], tr[self.ofr], pos[self.opt], self.uv, want_jac)

    def cost(self, x):
        """(cost, finite)"""
        r, _, c = self.evaluate(x, False)
        return float(c.sum()), bool(np.all(np.isfinite(r)) and np.all(np.isfinite(c)))

    def linearize(self, x):
        """dense J (2 n_obs x nu), r, cost"""
        r, Jo, c = self.evaluate(x)
        n = len(self.ofr)
        J = np.zeros((2 * n, self.nu))
        rows = np.arange(n)
        for row in range(2):
            for k in range(3):
                cr = self.col_rot[self.ofr]; m = cr >= 0
                J[2 * rows[m] + row, cr[m] + k] = Jo[m, row, k]
                ct = self.col_tr[self.ofr]; m = ct >= 0
                J[2 * rows[m] + row, ct[m] + k] = Jo[m, row, 3 + k]
                J[2 * rows + row, self.nc + 3 * self.opt + k] = Jo[:, row, 6 + k]
        return J, r.reshape(-1), float(c.sum())

    def plus(self, x, delta):
        rot, tr, pos = (a.copy() for a in x)
        for f in range(self.F):
            if self.col_rot[f] >= 0:
                rot[f] = quat_plus(x[0][f], delta[self.col_rot[f]:self.col_rot[f] + 3])
            if self.col_tr[f] >= 0:
                tr[f] = x[1][f] + delta[self.col_tr[f]:self.col_tr[f] + 3]
        pos = x[2] + delta[self.nc:].reshape(-1, 3)
        return (rot, tr, pos)

    def free_coordinates(self, x):
        """the ambient coordinates of the non-constant blocks, concatenated"""
        return np.concatenate([x[0][self.col_rot >= 0].ravel(), x[1][self.col_tr >= 0].ravel(), x[2].ravel()])


def _triangular_solve(L, b, trans):
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, b, lower=True, trans=1 if trans else 0)
    except ImportError:
        return np.linalg.solve(L.T if trans else L, b)


def world_frame(c_rotation, c_translation):
    """:290-303 in the order include/tcv_sfm_ba.h states: q[i] = c_rotation[i]^-1 (Eigen inverse()), T[i] = -(q[i] * c_translation[i])"""
    r, c = np.asarray(c_rotation, float), np.asarray(c_translation, float)
    n = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3]
    w, x, y, z = r[:, 0] / n, -r[:, 1] / n, -r[:, 2] / n, -r[:, 3] / n
    u0, u1, u2 = 2.0 * (y * c[:, 2] - z * c[:, 1]), 2.0 * (z * c[:, 0] - x * c[:, 2]), 2.0 * (x * c[:, 1] - y * c[:, 0])
    T = np.stack([-((c[:, 0] + w * u0) + (y * u2 - z * u1)), -((c[:, 1] + w * u1) + (z * u0 - x * u2)), -((c[:, 2] + w * u2) + (x * u1 - y * u0))], 1)
    return np.stack([w, x, y, z], 1), T


def solve(p, ceres=None):
    """ceres::Solve of :279 and what follows it.  ceres: CERES_DEFAULTS overrides (max_num_iterations among them).
    Returns dict(c_rotation, c_translation, position, q, T, summary) with summary = dict(iterations=[records], termination, termination_code,
    initial_cost, final_cost, accepted, num_camera_unknowns, num_points, num_observations).  A record of a valid step also carries what its
    decisions compare (decision_margin): model_cost_change, step_norm, x_norm, and gradient_max after an accepted step (the first: at entry)."""
    C = dict(CERES_DEFAULTS, **(ceres or {}))
    G = Problem(p)
    x = G.x0()
    summary = dict(termination="NO_CONVERGENCE", num_camera_unknowns=G.nc, num_points=G.P, num_observations=len(G.ofr))
    its = []
    cost, finite = G.cost(x)
    if not finite:      # the initial evaluation fails: FAILURE, the state as given
        summary["termination"] = "FAILURE"
        cost = DBL_MAX
    else:
        J, r, cost = G.linearize(x)
        its.append(dict(cost=cost, cost_candidate=0.0, rho=0.0, radius=C["initial_trust_region_radius"], step=1))
        scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))      # jacobi scaling, fixed at iteration 0, over every column
        gmax = float(np.max(np.abs(J.T @ r)))
        its[0]["gradient_max"] = gmax
        radius, dec, invalid, it = C["initial_trust_region_radius"], 2.0, 0, 0
        done = gmax <= C["gradient_tolerance"]
        if done:
            summary["termination"] = "CONVERGENCE_GRADIENT"
        Js = JtJ = None
        while not done:
            if it >= C["max_num_iterations"]:
                break
            if radius < C["min_trust_region_radius"]:
                summary["termination"] = "CONVERGENCE_RADIUS"; break
            it += 1
            if Js is None:
                Js = J * scale
                JtJ = Js.T @ Js
            diag = np.clip(np.diag(JtJ), C["min_lm_diagonal"], C["max_lm_diagonal"])
            D = np.sqrt(diag / radius)
            step, valid = None, True
            try:
                Lc = np.linalg.cholesky(JtJ + np.diag(D * D))
                y = _triangular_solve(Lc, _triangular_solve(Lc, Js.T @ r, False), True)
                step = -y
                valid = bool(np.all(np.isfinite(step)))
            except np.linalg.LinAlgError:
                valid = False
            if valid:
                Jstep = Js @ step
                mcc = -float(Jstep @ (r + Jstep / 2.0))
                valid = mcc > 0.0
            if not valid:
                invalid += 1
                its.append(dict(cost=cost, cost_candidate=0.0, rho=0.0, radius=radius, step=-1))
                if invalid >= C["max_num_consecutive_invalid_steps"]:
                    summary["termination"] = "FAILURE"; break
                radius *= 0.5
                continue
            invalid = 0
            xc = G.plus(x, step * scale)
            cand, cand_finite = G.cost(xc)
            if not cand_finite:
                cand = DBL_MAX
            dxn = float(np.linalg.norm(G.free_coordinates(xc) - G.free_coordinates(x))); xn = float(np.linalg.norm(G.free_coordinates(x)))
            cc = cost - cand
            rho = cc / mcc
            rec = dict(cost_candidate=cand, rho=rho, radius=radius, model_cost_change=mcc, step_norm=dxn, x_norm=xn, candidate_finite=cand_finite)
            if dxn <= C["parameter_tolerance"] * (xn + C["parameter_tolerance"]):
                its.append(dict(rec, cost=cost, step=0)); summary["termination"] = "CONVERGENCE_PARAMETER"; break
            if abs(cc) <= C["function_tolerance"] * cost:
                its.append(dict(rec, cost=cost, step=0)); summary["termination"] = "CONVERGENCE_FUNCTION"; break
            if rho > C["min_relative_decrease"]:
                x = xc
                J, r, cost = G.linearize(x)
                Js = None
                cost = cand
                gmax = float(np.max(np.abs(J.T @ r)))
                its.append(dict(rec, cost=cost, step=1, gradient_max=gmax))
                radius = min(C["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                dec = 2.0
                if gmax <= C["gradient_tolerance"]:
                    summary["termination"] = "CONVERGENCE_GRADIENT"; break
            else:
                its.append(dict(rec, cost=cost, step=0))
                radius /= dec; dec *= 2.0
    initial = its[0]["cost"] if its else DBL_MAX
    summary.update(iterations=its, termination_code=TERMINATION_CODE[summary["termination"]], initial_cost=initial, final_cost=cost,
                   accepted=bool(summary["termination"].startswith("CONVERGENCE") or cost < ACCEPT_COST))
    q, T = world_frame(x[0], x[1])
    return dict(c_rotation=x[0], c_translation=x[1], position=x[2], q=q, T=T, summary=summary)


# ------------------------------------------------------------------------------------------------ seeded test observations
def random_observations(rng, n):
    """n observations (rotation, translation, point, uv): every fourth quaternion with w < 0, every third of norm 1 +- 1e-3, every fifth
    point next to the image plane's edge (|u| about 1: a field of view of 90 degrees)"""
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[:, 0] = np.abs(q[:, 0]); q[::4, 0] *= -1.0
    q[::3] *= (1.0 + 1e-3 * np.where(np.arange(len(q[::3])) % 2, 1.0, -1.0))[:, None]
    t = rng.normal(0, 0.5, (n, 3))
    pc = np.column_stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), np.ones(n)]) * rng.uniform(4, 9, n)[:, None]      # in the camera
    pc[::5, 0] = pc[::5, 2] * rng.uniform(0.95, 1.05, len(pc[::5]))
    R = quat_matrix(q)
    X = np.einsum("nji,nj->ni", R, pc - t)
    uv = pc[:, :2] / pc[:, 2:3] + rng.normal(0, 0.01, (n, 2))
    return q, t, X, uv


# ------------------------------------------------------------------------------------------------ seeded test problems
def rotvec_quat(v):
    """unit quaternion (w x y z) of a rotation vector"""
    a = float(np.linalg.norm(v))
    return np.array([1.0, 0, 0, 0]) if a == 0 else np.concatenate([[np.cos(a / 2)], np.sin(a / 2) / a * np.asarray(v)])


def make_problem(seed, F=11, n_points=100, l=0, pose_noise=0.02, point_noise=0.05, pixel_noise=1.0 / 460.0, visible=0.7, min_obs=2, see=None,
                 blind_frames=(), only_frames=None):
    """Cameras along a smooth arc looking ahead, points 4 .. 9 m in front of them, each point seen by a random subset of at least `min_obs`
    frames (`visible`: the chance of each further frame), pixel noise, and the poses and points perturbed from the truth.  Frame l and the
    translation of frame F - 1 keep their true values (they are the constants that fix the gauge and the scale).
    see: per point the exact list of frames (overrides the random subset); blind_frames: frames no point sees; only_frames: the frames the
    random subsets are drawn from."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0.0, 0.35, F) + rng.normal(0, 0.01, F)
    centre = np.column_stack([3.0 * np.sin(ang), 0.05 * rng.normal(size=F), 3.0 * (1 - np.cos(ang))])      # world
    rot_true = np.array([quat_product(rotvec_quat(rng.normal(0, 0.02, 3)), rotvec_quat([0.0, -a, 0.0])) for a in ang])      # camera from world
    R_true = quat_matrix(rot_true)
    tr_true = -np.einsum("nij,nj->ni", R_true, centre)
    mid = F // 2
    pc = np.column_stack([rng.uniform(-0.35, 0.35, n_points), rng.uniform(-0.3, 0.3, n_points), np.ones(n_points)]) * rng.uniform(4, 9, n_points)[:, None]
    X_true = (pc - tr_true[mid]) @ R_true[mid]      # R^T (pc - t)
    pool = [f for f in (range(F) if only_frames is None else only_frames) if f not in blind_frames]
    obs = []
    for k in range(n_points):
        if see is not None and k < len(see) and see[k] is not None:
            frames = list(see[k])
        else:
            first = list(rng.choice(pool, min(min_obs, len(pool)), replace=False))
            frames = sorted(set(first) | {f for f in pool if rng.random() < visible})
        po = []
        for f in frames:
            p = R_true[f] @ X_true[k] + tr_true[f]
            po.append((int(f), float(p[0] / p[2] + rng.normal(0, pixel_noise)), float(p[1] / p[2] + rng.normal(0, pixel_noise))))
        obs.append(po)
    rot = rot_true.copy(); tr = tr_true.copy()
    for f in range(F):
        if f != l:
            rot[f] = quat_product(rotvec_quat(rng.normal(0, pose_noise, 3)), rot_true[f])
            if f != F - 1:
                tr[f] = tr_true[f] + rng.normal(0, pose_noise, 3)
    X = X_true + rng.normal(0, point_noise, (n_points, 3))
    return dict(c_rotation=rot, c_translation=tr, l=l, position=X, observations=obs)


def with_point_on_camera_plane(p, point=0):
    """a copy whose point `point` lies exactly on the plane z = 0 of the first camera that sees it: the residual there is not finite"""
    q = dict(p, position=np.array(p["position"], float))
    f = p["observations"][point][0][0]
    R = quat_matrix(np.asarray(p["c_rotation"], float)[f:f + 1])[0]
    t = np.asarray(p["c_translation"], float)[f]
    q["position"][point] = R.T @ (np.array([0.3, -0.2, 0.0]) - t)
    # (rounding may leave p_z at 1e-17 instead of 0: move the point along the optical axis until it is exact)
    for _ in range(60):
        pz = float(R[2] @ q["position"][point] + t[2])
        if pz == 0.0:
            break
        q["position"][point] = q["position"][point] - pz * R[2]
    return q


# name -> make_problem arguments; the seeds were chosen on the CPU so that every decision of the oracle's solve is at least 1e-3 (relative)
# from its threshold and each named path is reached (tests/test_sfm_ba_cpu.py holds them to that)
TEST_PROBLEMS = dict(
    f11_l0_p40=dict(seed=1, F=11, n_points=40, l=0),
    f11_l5_p90=dict(seed=2, F=11, n_points=90, l=5),
    f11_l9_p150=dict(seed=3, F=11, n_points=150, l=9),
    f2_l0=dict(seed=4, F=2, n_points=30, l=0, visible=1.0),
    f3_l1=dict(seed=5, F=3, n_points=30, l=1),
    exact=dict(seed=6, F=11, n_points=40, l=3, pose_noise=0.0, point_noise=0.0, pixel_noise=0.0),
    one_point_six_frames=dict(seed=1, F=6, n_points=1, l=0, see=[[0, 1, 2, 3, 4, 5]]),
    two_and_all=dict(seed=8, F=11, n_points=20, l=0, see=[[2, 7], list(range(11))]),
    idle_frame=dict(seed=9, F=11, n_points=40, l=0, blind_frames=(4,)),
    constant_frames_only=dict(seed=10, F=11, n_points=30, l=2, see=[[2, 10]] * 6),
    rejected=dict(seed=17, F=11, n_points=60, l=0, pose_noise=0.15, point_noise=0.6),
    no_convergence=dict(seed=16, F=11, n_points=60, l=0, pose_noise=0.3, point_noise=1.5),
)


def test_problems():
    """the problems of the solve-level tests, by name"""
    return {k: make_problem(**kw) for k, kw in TEST_PROBLEMS.items()}


# (F, l, points) on and next to every size built into the kernel (csrc/tcv_sfm_ba.h: BA_CHUNK 16 points per staged chunk, 256 threads over
# the points, tiles of 4 over the nc + 1 rows of the reduced camera system, TCV_SFM_BA_MAX_POINTS, TCV_SFM_BA_MAX_FRAMES)
BOUNDARY_SHAPES = [
    (3, 1, 1), (3, 1, 15), (3, 1, 16), (3, 1, 17),       # nc 9; one partial chunk, exactly one, one and a point
    (4, 0, 31), (4, 0, 32), (4, 0, 33),                  # nc 15: nc + 1 = 16 fills its tiles exactly; two chunks
    (2, 0, 48), (3, 2, 48),                              # nc 3: one tile; nc 12 (l = F - 1): 13 rows in 16
    (11, 5, 255), (11, 5, 256), (11, 5, 257),            # the 256 point owners: one pass, and a second one for one point
    (15, 14, 40), (15, 3, 40),                           # TCV_SFM_BA_MAX_FRAMES: nc 84 (the widest system, 88 x 88 with 253 tiles) and 81
    (3, 1, 1024),                                        # TCV_SFM_BA_MAX_POINTS
]
BOUNDARY_SEEDS = {shape: 200 + i for i, shape in enumerate(BOUNDARY_SHAPES)}


def boundary_problems():
    """name -> problem for BOUNDARY_SHAPES"""
    out = {}
    for (F, l, n) in BOUNDARY_SHAPES:
        kw = dict(visible=0.5) if n >= 1024 else {}
        out["f%d_l%d_p%d" % (F, l, n)] = make_problem(BOUNDARY_SEEDS[(F, l, n)], F=F, n_points=n, l=l, **kw)
    return out
