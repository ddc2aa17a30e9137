"""NumPy restatement of PoseGraph::optimize4DoF (reference pose_graph/src/pose_graph.cpp:403-579, cost functors and the angle
parameterisation pose_graph.h:89-246): the graph construction of :445-519, the two edges with analytic Jacobians, Ceres' trust-region
loop with LevenbergMarquardtStrategy, and the drift of :549-557.  Test infrastructure: dense numpy.linalg for the step.

Like the rest of the oracles it is UNPINNED against a real Ceres: upstream Ceres 2.x as read, every default it
relies on by name in CERES_DEFAULTS below (the shared ones come from np_oracle.CERES_DEFAULTS)."""
from __future__ import annotations

import numpy as np

import np_oracle as NO

CERES_DEFAULTS = dict(
    {k: NO.CERES_DEFAULTS[k] for k in ("jacobi_scaling", "min_lm_diagonal", "max_lm_diagonal", "initial_trust_region_radius", "min_relative_decrease",
                                       "function_tolerance", "parameter_tolerance", "gradient_tolerance", "min_trust_region_radius",
                                       "max_num_consecutive_invalid_steps")},
    max_trust_region_radius=1e16,
    lm_step_accepted="radius / max(1/3, 1 - (2 rho - 1)^3)",      # LevenbergMarquardtStrategy::StepAccepted, decrease_factor back to 2
    lm_step_rejected="radius / decrease_factor; decrease_factor *= 2",
    lm_step_invalid="radius / 2",                                 # StepIsInvalid
    corrector="alpha = 0 where rho'' <= 0",                       # Corrector: Huber never has rho'' > 0
)
REFERENCE_OPTIONS = dict(max_num_iterations=5, huber_delta=0.1, loop_weight=1.0, loop_yaw_divisor=10.0)      # pose_graph.cpp:437, :440; pose_graph.h:207, :231
TERMINATION_CODE = NO.TERMINATION_CODE


def normalize_angle(a):      # pose_graph.h:89-97, one wrap
    return a - 360.0 if a > 180.0 else (a + 360.0 if a < -180.0 else a)


def r2ypr(R):      # Utility::R2ypr, degrees
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return np.array([y, p, r]) / np.pi * 180.0


def ypr2R(y, p, r):      # Utility::ypr2R, degrees
    y, p, r = np.array([y, p, r]) / 180.0 * np.pi
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1.0, 0], [-np.sin(p), 0, np.cos(p)]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return Rz @ Ry @ Rx


def q2R(q):      # Eigen toRotationMatrix, q = x y z w, not normalised
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def R2q(R):
    """a unit quaternion (x y z w) of a rotation matrix (test helper)"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    return np.array([x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), (R[2, 1] - R[1, 2]) / (4 * x)])


def edge(kind, xi, xj, meas, opt=REFERENCE_OPTIONS, correct=True, want_jac=True):
    """FourDOFError (kind 0) / FourDOFWeightError (kind 1) between x_i = (yaw, t) and x_j; meas = relative_t 3, relative_yaw, pitch_i, roll_i.
    Returns cost (rho / 2), residual (4), J_i (4 x 4), J_j (4 x 4); with `correct` the last three as Ceres' corrector leaves them."""
    k = np.pi / 180.0
    y, p, ro = xi[0] * k, meas[4] * k, meas[5] * k
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(ro), np.sin(ro)
    R = np.array([[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr], [-sp, cp * sr, cp * cr]])
    dR = np.array([[-sy * cp, -cy * cr - sy * sp * sr, cy * sr - sy * sp * cr], [cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [0, 0, 0]]) * k
    d = np.asarray(xj[1:4]) - np.asarray(xi[1:4])
    w = opt["loop_weight"] if kind else 1.0
    wy = opt["loop_weight"] / opt["loop_yaw_divisor"] if kind else 1.0
    r = np.empty(4)
    r[:3] = (R.T @ d - np.asarray(meas[:3])) * w
    r[3] = normalize_angle(xj[0] - xi[0] - meas[3]) * wy
    s = float(r @ r)
    cost, c = 0.5 * s, 1.0
    a = opt["huber_delta"]
    if kind and a > 0 and s > a * a:      # HuberLoss::Evaluate
        cost = 0.5 * (2 * a * np.sqrt(s) - a * a)
        c = np.sqrt(max(np.finfo(float).tiny, a / np.sqrt(s)))
    if not correct:
        c = 1.0
    if not want_jac:
        return cost, c * r, None, None
    Ji = np.zeros((4, 4)); Jj = np.zeros((4, 4))
    Ji[:3, 0] = w * (dR.T @ d); Ji[:3, 1:] = -w * R.T; Jj[:3, 1:] = w * R.T
    Ji[3, 0] = -wy; Jj[3, 0] = wy
    return cost, c * r, c * Ji, c * Jj


class Graph:
    """the problem of :445-519 over dict(t, q (xyzw), sequence or None, loops [(cur, old, relative_t, relative_yaw)])"""

    def __init__(self, g, opt=None):
        self.opt = dict(REFERENCE_OPTIONS, **(opt or {}))
        self.t = np.asarray(g["t"], float).reshape(-1, 3)
        self.q = np.asarray(g["q"], float).reshape(-1, 4)
        N = self.N = len(self.t)
        seq = g.get("sequence")
        self.seq = np.ones(N, int) if seq is None else np.asarray(seq, int)
        self.ypr = np.array([r2ypr(q2R(self.q[i])) for i in range(N)])
        self.const = np.array([i == 0 or self.seq[i] == 0 for i in range(N)])
        self.edges = []      # (kind, a, b, meas)
        loops = list(g.get("loops", []))
        for i in range(N):
            for j in range(1, 5):
                if i - j >= 0 and self.seq[i] == self.seq[i - j]:
                    a = i - j
                    qa = self.q[a]
                    Rinv = q2R(np.array([-qa[0], -qa[1], -qa[2], qa[3]]) / float(qa @ qa))
                    rel = Rinv @ (self.t[i] - self.t[a])
                    self.edges.append((0, a, i, np.array([rel[0], rel[1], rel[2], self.ypr[i, 0] - self.ypr[a, 0], self.ypr[a, 1], self.ypr[a, 2]])))
            for (cur, old, rt, ryaw) in loops:
                if cur == i:
                    self.edges.append((1, old, i, np.array([rt[0], rt[1], rt[2], ryaw, self.ypr[old, 1], self.ypr[old, 2]])))
        self.free = [i for i in range(N) if not self.const[i]]
        self.col = {n: 4 * k for k, n in enumerate(self.free)}
        self.red = [e for e in self.edges if not (self.const[e[1]] and self.const[e[2]])]
        self.fixed = [e for e in self.edges if self.const[e[1]] and self.const[e[2]]]

    def x0(self):
        return np.column_stack([self.ypr[:, 0], self.t])

    def cost(self, x, edges=None):
        return float(sum(edge(k, x[a], x[b], m, self.opt, want_jac=False)[0] for (k, a, b, m) in (self.red if edges is None else edges)))

    def linearize(self, x):
        nf = 4 * len(self.free)
        J = np.zeros((4 * len(self.red), nf)); r = np.zeros(4 * len(self.red)); cost = 0.0
        for n, (k, a, b, m) in enumerate(self.red):
            c, re, Ja, Jb = edge(k, x[a], x[b], m, self.opt)
            cost += c; r[4 * n:4 * n + 4] = re
            if not self.const[a]:
                J[4 * n:4 * n + 4, self.col[a]:self.col[a] + 4] = Ja
            if not self.const[b]:
                J[4 * n:4 * n + 4, self.col[b]:self.col[b] + 4] = Jb
        return J, r, float(cost)

    def plus(self, x, delta):
        xc = x.copy()
        for n in self.free:
            d = delta[self.col[n]:self.col[n] + 4]
            xc[n, 0] = normalize_angle(x[n, 0] + d[0]); xc[n, 1:] = x[n, 1:] + d[1:]
        return xc


def solve(g, opt=None, ceres=None):
    """ceres::Solve of :522 and what follows it.  opt: REFERENCE_OPTIONS overrides; ceres: CERES_DEFAULTS overrides.
    Returns dict(t, R, x, summary) with summary = dict(iterations=[records], termination, termination_code, initial_cost, final_cost,
    yaw_drift, r_drift, t_drift, num_free_nodes, num_edges).  A record of a valid step also carries what its decisions compare
    (decision_margin below): model_cost_change, step_norm and x_norm of the parameter test, and gradient_max after an accepted step
    (the first record: at entry)."""
    C = dict(CERES_DEFAULTS, **(ceres or {}))
    G = Graph(g, opt)
    x = G.x0()
    fixed_cost = G.cost(x, G.fixed)
    summary = dict(termination="NO_CONVERGENCE", num_free_nodes=len(G.free), num_edges=len(G.red))
    its = []
    free = np.array(G.free, int)
    if len(G.free) == 0:
        cost = G.cost(x)
        its.append(dict(cost=cost, cost_candidate=0.0, rho=0.0, radius=C["initial_trust_region_radius"], step=1))
        summary["termination"] = "CONVERGENCE_GRADIENT"
    else:
        J, r, cost = G.linearize(x)
        its.append(dict(cost=cost, cost_candidate=0.0, rho=0.0, radius=C["initial_trust_region_radius"], step=1))
        scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))      # jacobi scaling, fixed at iteration 0
        gmax = float(np.max(np.abs(J.T @ r)))
        its[0]["gradient_max"] = gmax
        radius, dec, invalid, it = C["initial_trust_region_radius"], 2.0, 0, 0
        done = gmax <= C["gradient_tolerance"]
        if done:
            summary["termination"] = "CONVERGENCE_GRADIENT"
        while not done:
            if it >= G.opt["max_num_iterations"]:
                break
            if radius < C["min_trust_region_radius"]:
                summary["termination"] = "CONVERGENCE_RADIUS"; break
            it += 1
            Js = J * scale
            diag = np.clip((Js * Js).sum(0), C["min_lm_diagonal"], C["max_lm_diagonal"])
            D = np.sqrt(diag / radius)
            step, valid = None, True
            try:
                Lc = np.linalg.cholesky(Js.T @ Js + np.diag(D * D))
                y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, Js.T @ r))
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
            delta = step * scale
            xc = G.plus(x, delta)
            cand = G.cost(xc)
            dxn = np.linalg.norm((xc - x)[free]); xn = np.linalg.norm(x[free])
            cc = cost - cand
            rho = cc / mcc
            rec = dict(cost_candidate=cand, rho=rho, radius=radius, model_cost_change=mcc, step_norm=float(dxn), x_norm=float(xn))
            if dxn <= C["parameter_tolerance"] * (xn + C["parameter_tolerance"]):
                its.append(dict(rec, cost=cost, step=0)); summary["termination"] = "CONVERGENCE_PARAMETER"; break
            if abs(cc) <= C["function_tolerance"] * cost:
                its.append(dict(rec, cost=cost, step=0)); summary["termination"] = "CONVERGENCE_FUNCTION"; break
            if rho > C["min_relative_decrease"]:
                x = xc
                J, r, cost = G.linearize(x)
                gmax = float(np.max(np.abs(J.T @ r)))
                its.append(dict(rec, cost=cost, step=1, gradient_max=gmax))
                radius = min(C["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                dec = 2.0
                if gmax <= C["gradient_tolerance"]:
                    summary["termination"] = "CONVERGENCE_GRADIENT"; break
            else:
                its.append(dict(rec, cost=cost, step=0))
                radius /= dec; dec *= 2.0
    N = G.N
    R = np.array([ypr2R(x[i, 0], G.ypr[i, 1], G.ypr[i, 2]) for i in range(N)])
    yaw_drift = r2ypr(R[N - 1])[0] - G.ypr[N - 1, 0]
    r_drift = ypr2R(yaw_drift, 0, 0)
    t_drift = x[N - 1, 1:] - r_drift @ G.t[N - 1]
    summary.update(iterations=its, termination_code=TERMINATION_CODE[summary["termination"]], initial_cost=its[0]["cost"] + fixed_cost,
                   final_cost=cost + fixed_cost, yaw_drift=float(yaw_drift), r_drift=r_drift, t_drift=t_drift)
    return dict(t=x[:, 1:].copy(), R=R, x=x, summary=summary)


def decision_margin(summary, ceres=None):
    """How close a solve came to deciding otherwise: the smallest |quantity / threshold - 1| over every floating-point comparison the loop
    made, as (margin, what, record).  In the order of the loop, per record of a valid step: step_norm against parameter_tolerance * (x_norm +
    parameter_tolerance); |cost change| against function_tolerance * cost; rho against min_relative_decrease; after an accepted step (and
    at entry) gradient_max against gradient_tolerance.  A comparison the loop did not reach, or whose threshold is zero, is left out.
    An invalid step (a pivot or model_cost_change not positive) is a margin of 0: it compares against zero."""
    C = dict(CERES_DEFAULTS, **(ceres or {}))
    best = (np.inf, "none", 0)

    def see(q, thr, what, n):
        nonlocal best
        if thr > 0.0 and abs(q / thr - 1.0) < best[0]:
            best = (abs(q / thr - 1.0), what, n)

    its = summary["iterations"]
    for n, rec in enumerate(its):
        if rec["step"] < 0:
            return 0.0, "invalid step", n
        if n > 0:
            cost_before = its[n - 1]["cost"] if rec["step"] == 1 else rec["cost"]      # (an accepted step's record holds the new cost)
            see(rec["step_norm"], C["parameter_tolerance"] * (rec["x_norm"] + C["parameter_tolerance"]), "parameter_tolerance", n)
            if n == len(its) - 1 and summary["termination"] == "CONVERGENCE_PARAMETER":
                break
            see(abs(cost_before - rec["cost_candidate"]), C["function_tolerance"] * cost_before, "function_tolerance", n)
            if n == len(its) - 1 and summary["termination"] == "CONVERGENCE_FUNCTION":
                break
            see(rec["rho"], C["min_relative_decrease"], "min_relative_decrease", n)
        if "gradient_max" in rec:
            see(rec["gradient_max"], C["gradient_tolerance"], "gradient_tolerance", n)
    return best


# ------------------------------------------------------------------------------------------------ seeded test edges
def random_edge(rng, kind, wrap=0, big_tilt=False, huber=None):
    """one edge; wrap +-1: yaw_j - yaw_i - relative_yaw just beyond +-180; huber True / False: |r|^2 above / below huber_delta^2"""
    xi = np.concatenate([[rng.uniform(-180, 180)], rng.normal(0, 3, 3)])
    xj = np.concatenate([[rng.uniform(-180, 180)], xi[1:] + rng.normal(0, 1, 3)])
    tilt = 60.0 if big_tilt else 10.0
    pitch, roll = rng.uniform(-tilt, tilt, 2)
    R = ypr2R(xi[0], pitch, roll)
    amp = {None: 0.05, True: 0.5, False: 0.005}[huber]
    rel_t = R.T @ (xj[1:] - xi[1:]) + rng.normal(0, amp, 3)
    rel_yaw = xj[0] - xi[0] + rng.normal(0, amp)
    if wrap:
        rel_yaw = xj[0] - xi[0] - wrap * (180.0 + rng.uniform(0.01, 0.3))
    return kind, xi, xj, np.concatenate([rel_t, [rel_yaw, pitch, roll]])


# ------------------------------------------------------------------------------------------------ seeded test graphs
def make_graph(seed, n, loops=(), sequence=None, yaw0=0.0, drift=0.02, loop_noise=0.0, bad_loops=()):
    """A trajectory with ground truth and a drifting VIO copy of it.  loops: (cur, old) pairs measured on the ground truth (+ loop_noise);
    bad_loops: indices into `loops` whose measurement is grossly wrong."""
    rng = np.random.default_rng(seed)
    yaw = yaw0 + np.cumsum(rng.normal(4.0, 2.0, n))
    pitch = rng.normal(0, 5.0, n); roll = rng.normal(0, 5.0, n)
    t = np.cumsum(rng.normal(0.0, 0.3, (n, 3)) + np.array([0.4, 0.1, 0.0]), axis=0)
    # VIO: accumulated drift in yaw and position
    yaw_v = yaw + np.cumsum(rng.normal(drift * 10, drift * 5, n)); t_v = t + np.cumsum(rng.normal(drift, drift, (n, 3)), axis=0)
    wrap = lambda a: (a + 180.0) % 360.0 - 180.0
    q = np.array([R2q(ypr2R(wrap(yaw_v[i]), pitch[i], roll[i])) for i in range(n)])
    L = []
    for k, (cur, old) in enumerate(loops):
        Ro = ypr2R(wrap(yaw[old]), pitch[old], roll[old])
        rt = Ro.T @ (t[cur] - t[old]) + rng.normal(0, loop_noise, 3)
        ry = wrap(yaw[cur] - yaw[old]) + rng.normal(0, loop_noise * 10)
        if k in bad_loops:
            rt = rt + np.array([3.0, -2.0, 1.0]); ry = ry + 25.0
        L.append((int(cur), int(old), rt, float(ry)))
    return dict(t=t_v, q=q, sequence=None if sequence is None else np.asarray(sequence, int), loops=L)


def test_graphs():
    """the graphs of the solve-level tests, by name"""
    G = {}
    G["n1"] = make_graph(1, 1)
    G["n2"] = make_graph(2, 2, [(1, 0)])
    G["n5"] = make_graph(3, 5, [(4, 1)])
    G["n6"] = make_graph(4, 6, [(5, 1)])
    G["n12_const_and_free_old"] = make_graph(5, 12, [(11, 0), (10, 2)])
    G["n12_loop_in_band"] = make_graph(6, 12, [(7, 5)])
    G["n16_consecutive_borders"] = make_graph(7, 16, [(12, 1), (13, 2), (14, 3), (15, 4)])
    G["n16_shared_newer"] = make_graph(8, 16, [(14, 2), (14, 5)])
    G["n20_sequences"] = make_graph(9, 20, [(18, 5), (12, 6), (3, 1), (8, 2)], sequence=[0] * 4 + [1] * 6 + [2] * 10)
    G["n12_yaw_wrap"] = make_graph(10, 12, [(11, 1)], yaw0=150.0)
    G["n12_huber"] = make_graph(11, 12, [(10, 1), (11, 3)], bad_loops=(1,))
    G["n12_no_loops"] = make_graph(12, 12)
    rng = np.random.default_rng(13)
    cur = rng.choice(np.arange(60, 300), 40, replace=False)
    G["n300"] = make_graph(13, 300, [(int(c), int(rng.integers(1, c - 30))) for c in sorted(cur)], drift=0.005, loop_noise=0.01)
    return G


# ------------------------------------------------------------------------------------------------ graphs of a chosen shape
def shape_graph(seed, nb, nk, **make_graph_kw):
    """A graph whose elimination order is (free, band, border) = (nb + nk, nb, nk): node 0 constant, nodes 1 .. nb the band, each of the
    last nk nodes the newer end of one loop whose older end is the free node 1 + (3 k mod nb).  Without a border a loop (two when nb > 6) to
    the constant node 0 gives the problem a residual and makes no border; without any loop the solve would end at entry."""
    n = 1 + nb + nk
    loops = []
    for k in range(nk):
        cur, old = 1 + nb + k, 1 + (3 * k) % nb
        loops.append((cur, old if old < cur else 1))
    if nk == 0:
        loops.append((nb, 0))
        if nb > 6:
            loops.append((nb // 2 + 1, 0))
    return make_graph(seed, n, loops, **dict(dict(drift=0.01, loop_noise=0.005), **make_graph_kw))


# (nb, nk) on and next to every size built into the kernel; the unknowns are nbs = 4 nb in the band, m = 4 nk in the border, the border
# has M1 = m + 1 rows with the right-hand side (csrc/tcv_pose_graph.hip: PG_LD 20, PG_KC 32, PG_PANEL_COLS 301, PG_PANEL_ROWS 320, Schur
# tiles of 64, 256 threads)
BOUNDARY_SHAPES = [
    (1, 0), (2, 0), (4, 0),              # nbs 4, 8, 16 < PG_LD: narrower than the half-bandwidth, one partial substitution chunk
    (5, 0), (6, 0),                      # nbs 20: exactly one chunk; 24: one and a partial one
    (8, 1), (9, 16),                     # nbs 32 = PG_KC, 36; (8, 1) the smallest border
    (75, 0), (76, 0),                    # nbs 300: the last size of one panel; 304: a second panel of three columns, a node across the seam
    (80, 0), (81, 0),                    # nbs 320 = PG_PANEL_ROWS, 324
    (150, 0), (151, 0),                  # nbs 600, 604: a third panel of two columns
    (1, 2), (5, 5),                      # the border larger than / as large as the band
    (8, 15), (8, 16), (8, 17),           # m 60, 64, 68 around one Schur tile
    (8, 63), (8, 64), (9, 65),           # M1 253, 257, 261 around the 256-thread row loops
    (12, 128), (8, 256),                 # m 512; m 1024 with TCV_POSE_GRAPH_MAX_LOOPS loops
    (76, 17), (81, 64),                  # a panel seam and a tile edge in one graph
]
# seed per shape: every decision of the oracle's solve at least 1 % from its threshold (tests/test_pose_graph_cpu.py)
BOUNDARY_SEEDS = {shape: 100 + i for i, shape in enumerate(BOUNDARY_SHAPES)}
BOUNDARY_SEEDS.update({(12, 128): 300, (8, 256): 301})


def boundary_graphs():
    """name -> graph for BOUNDARY_SHAPES"""
    return {"b%d_k%d" % (nb, nk): shape_graph(BOUNDARY_SEEDS[(nb, nk)], nb, nk) for (nb, nk) in BOUNDARY_SHAPES}
