"""NumPy restatement of the visual-inertial alignment (include/tcv_vi_alignment.h) with the number format as a parameter (float64, long
double): solveGyroscopeBias, LinearAlignment, TangentBasis, RefineGravity (reference initial_aligment.cpp:3-197), the state change of
Estimator::visualInitialAlign (estimator.cpp:1380-1438) and Utility::g2R (utility.cpp:3-13).  It takes pre-integrations as input (dicts in
the layout of synth.preintegrate / tcv.preintegrate): `gyro_bias` those at (ba0, bg0), `align` those re-propagated at (0, bg).

The matrices are built dense, as the reference builds them; the solves are a hand-written Cholesky in natural order -- the kernel's
elimination order -- that records every relative pivot d_k / A_kk and stops at the first one that fails the gate.  `solver="dense"` solves
the same normal equations with numpy.linalg.solve instead (LU with partial pivoting: an elimination order of its own, as the reference's
pivoted LDLT has one); the tests use it only to size float64 rounding noise.

NON_FINITE sits where the kernel has it: after the bias solve, after LinearAlignment's s and g, after the refinement's s, g and x, each
with the header's zero pattern behind it.  `flags` counts the branches taken: TangentBasis's special case and g2R's antiparallel one."""
import numpy as np

OK, LINEAR, REFINED_SCALE, RANK, NON_FINITE = 0, 1, 2, 3, 4
PI = 3.14159265358979323846


def cholesky_solve(A, b, gate):
    """x of A x = b by an unpivoted right-looking Cholesky (None where pivot k has d_k <= gate * A_kk), and the relative pivots met"""
    return cholesky_solve_info(A, b, gate)[:2]


def dense_solve(A, b):
    """the second float64 solve: numpy.linalg.solve on the dense matrix (no gate, no pivots recorded)"""
    with np.errstate(all="ignore"):
        try:
            return np.linalg.solve(A.astype(np.float64), b.astype(np.float64)).astype(A.dtype)
        except np.linalg.LinAlgError:
            return None


def cholesky_solve_info(A, b, gate):
    """cholesky_solve, and A_kk of the pivot that failed (None where none did)"""
    A = A.copy(); y = b.copy()
    n = len(b)
    d0 = A.diagonal().copy()
    rel = []
    for j in range(n):
        d = A[j, j]
        rel.append(d / d0[j] if d0[j] != 0 else d * 0)
        if not d > gate * d0[j]:
            return None, np.array(rel, dtype=A.dtype), d0[j]
        l = np.sqrt(d)
        A[j, j] = l
        y[j] = y[j] / l
        nz = j + 1 + np.nonzero(A[j + 1:, j])[0]      # (structural zeros: no fill outside the band and the border)
        if len(nz):
            col = A[nz, j] / l
            A[nz, j] = col
            A[np.ix_(nz, nz)] -= np.outer(col, col)
            y[nz] -= col * y[j]
    x = y
    for j in range(n - 1, -1, -1):
        x[j] = x[j] / A[j, j]
        nz = np.nonzero(A[j, :j])[0]
        x[nz] -= A[j, nz] * x[j]
    return x, np.array(rel, dtype=A.dtype), None


# ------------------------------------------------------------------------------------------------ small rotation helpers, any dtype
def r2q(m):
    """Eigen's Quaterniond(Matrix3d), xyzw"""
    T = m.dtype.type
    q = np.zeros(4, m.dtype)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + T(1))
        q[3] = T(0.5) * t
        t = T(0.5) / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + T(1))
        q[i] = T(0.5) * t
        t = T(0.5) / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    return q


def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], dtype=a.dtype)


def qinv(q):
    n2 = q @ q
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=q.dtype) / n2


def q2R(q):
    x, y, z, w = q
    T = q.dtype.type
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=q.dtype) * T(1)


def r2ypr(R):
    """Utility::R2ypr (utility.h:70-85), degrees"""
    T = R.dtype.type
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return np.array([y, p, r], dtype=R.dtype) / T(PI) * T(180)


def ypr2R(ypr):
    """Utility::ypr2R (utility.h:87-112), degrees"""
    T = ypr.dtype.type
    y, p, r = ypr / T(180) * T(PI)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], dtype=ypr.dtype)
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], dtype=ypr.dtype)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], dtype=ypr.dtype)
    return Rz @ Ry @ Rx


def normalized(v):
    z = v @ v
    return v / np.sqrt(z) if z > 0 else v


def g2R_cos(g):
    """c of g2R: what decides its branch (antiparallel: c < -1 + 1e-12)"""
    return normalized(normalized(g)) @ np.array([0, 0, 1], dtype=g.dtype)


def g2R(g, flags=None):
    """Utility::g2R; FromTwoVectors with the fixed axis (1, 0, 0) in the antiparallel branch, as the kernel has it"""
    T = g.dtype.type
    v0 = normalized(normalized(g)); v1 = np.array([0, 0, 1], dtype=g.dtype)
    c = v1 @ v0
    if flags is not None:
        flags["g2R_c"] = c
    if c < T(-1) + T(1e-12):
        if flags is not None:
            flags["g2R_antiparallel"] = flags.get("g2R_antiparallel", 0) + 1
        w2 = max((T(1) + c) * T(0.5), T(0))
        q = np.array([np.sqrt(T(1) - w2), 0, 0, np.sqrt(w2)], dtype=g.dtype)
    else:
        axis = np.cross(v0, v1)
        s = np.sqrt((T(1) + c) * T(2))
        q = np.concatenate([axis * (T(1) / s), [s * T(0.5)]]).astype(g.dtype)
    R0 = q2R(q)
    yaw = r2ypr(R0)[0]
    return ypr2R(np.array([-yaw, 0, 0], dtype=g.dtype)) @ R0


def tangent_basis(g0, flags=None):
    a = normalized(g0)
    tmp = np.array([0, 0, 1], dtype=g0.dtype)
    if np.array_equal(a, tmp) or np.array_equal(a, -tmp):      # (the reference: a == tmp only; at -tmp its b is the zero vector -- DESIGN.md section 8)
        tmp = np.array([1, 0, 0], dtype=g0.dtype)
        if flags is not None:
            flags["tangent_special"] = flags.get("tangent_special", 0) + 1
    b = normalized(tmp - a * (a @ tmp))
    return np.stack([b, np.cross(a, b)], 1)


# ------------------------------------------------------------------------------------------------ the algorithm
def _finite(*xs):
    return all(bool(np.all(np.isfinite(np.asarray(x, dtype=np.float64)))) for x in xs)      # (an overflow of the cast is an overflow on the device too)


def _bias_system(R, pre0, dtype):
    R = np.asarray(R).reshape(-1, 3, 3).astype(dtype)
    T = np.dtype(dtype).type
    A = np.zeros((3, 3), dtype); b = np.zeros(3, dtype)
    for i in range(len(R) - 1):
        J = np.asarray(pre0["jacobian"][i])[3:6, 12:15].astype(dtype)
        q_ij = r2q(R[i].T @ R[i + 1])
        r = T(2) * qmul(qinv(np.asarray(pre0["delta_q"][i]).astype(dtype)), q_ij)[:3]
        A += J.T @ J; b += J.T @ r
    return A, b


def gyro_bias(R, pre0, dtype=np.float64, gate=0.0, solver="cholesky"):
    """solveGyroscopeBias (:3-27): delta_bg (None behind the gate) and the relative pivots"""
    A, b = _bias_system(R, pre0, dtype)
    if solver == "dense":
        return dense_solve(A, b), np.ones(0, dtype)
    return cholesky_solve(A, b, np.dtype(dtype).type(gate))


def gyro_bias_verdict(R, pre0, dtype=np.float64, gate=0.0):
    """(status, delta_bg, relative pivots, A_kk of the failed pivot): RANK behind the gate, NON_FINITE for a solution that is not finite, both
    with delta_bg zero -- what the bias kernel writes"""
    with np.errstate(all="ignore"):
        A, b = _bias_system(R, pre0, dtype)
        x, piv, a0 = cholesky_solve_info(A, b, np.dtype(dtype).type(gate))
    if x is None:
        return RANK, np.zeros(3, dtype), piv, a0
    if not _finite(x):
        return NON_FINITE, np.zeros(3, dtype), piv, None
    return OK, x, piv, None


def _system(R, Tr, tic, pre, nb, lxly, g0):
    """the normal equations of LinearAlignment (nb == 4, :125-178) or one round of RefineGravity (nb == 3, :63-116)"""
    dtype = R.dtype
    T = dtype.type
    F = len(R)
    n = 3 * F + nb
    A = np.zeros((n, n), dtype); b = np.zeros(n, dtype)
    I3 = np.eye(3, dtype=dtype)
    for i in range(F - 1):
        tA = np.zeros((6, 6 + nb), dtype); tb = np.zeros(6, dtype)
        dt = T(pre["sum_dt"][i]); dp = np.asarray(pre["delta_p"][i]).astype(dtype); dv = np.asarray(pre["delta_v"][i]).astype(dtype)
        Rit = R[i].T
        tA[0:3, 0:3] = -dt * I3
        tA[0:3, 6 + nb - 1] = Rit @ (Tr[i + 1] - Tr[i]) / T(100)
        tb[0:3] = dp + Rit @ R[i + 1] @ tic - tic
        tA[3:6, 0:3] = -I3
        tA[3:6, 3:6] = Rit @ R[i + 1]
        tb[3:6] = dv
        if nb == 4:
            tA[0:3, 6:9] = Rit * dt * dt / T(2)
            tA[3:6, 6:9] = Rit * dt
        else:
            tA[0:3, 6:8] = (Rit * dt * dt / T(2)) @ lxly
            tA[3:6, 6:8] = (Rit * dt) @ lxly
            tb[0:3] -= (Rit * dt * dt / T(2)) @ g0
            tb[3:6] -= (Rit * dt) @ g0
        rA = tA.T @ tA; rb = tA.T @ tb
        A[3 * i:3 * i + 6, 3 * i:3 * i + 6] += rA[:6, :6]; b[3 * i:3 * i + 6] += rb[:6]
        A[-nb:, -nb:] += rA[-nb:, -nb:]; b[-nb:] += rb[-nb:]
        A[3 * i:3 * i + 6, -nb:] += rA[:6, -nb:]; A[-nb:, 3 * i:3 * i + 6] += rA[-nb:, :6]
    return A * T(1000), b * T(1000)


def align(R, Tr, tic, pre, key_frame=None, gravity_norm=9.81007, dtype=np.float64, gate=0.0, solver="cholesky"):
    """LinearAlignment, RefineGravity and the state change; a dict with `status`, every quantity of tcv_vi_align_result that was computed (zeros
    behind it, as the header says), `pivots`, the relative pivots of every factorisation that ran, `stages`, the same stage by stage
    ("linear", "refine0" .. "refine3"; the first 3 F of a stage are the band's, the rest the border's), `fail_a0`, A_kk of a failed pivot, and
    `flags`, the branches taken"""
    with np.errstate(all="ignore"):
        return _align(R, Tr, tic, pre, key_frame, gravity_norm, dtype, gate, solver)


def _align(R, Tr, tic, pre, key_frame, gravity_norm, dtype, gate, solver):
    T = np.dtype(dtype).type
    R = np.asarray(R).reshape(-1, 3, 3).astype(dtype); Tr = np.asarray(Tr).reshape(-1, 3).astype(dtype); tic = np.asarray(tic).astype(dtype)
    F = len(R)
    key = np.arange(F) if key_frame is None else np.asarray(key_frame)
    K = len(key)
    G = T(gravity_norm)
    flags = {}
    zeros = dict(scale=T(0), gravity_c0=np.zeros(3, dtype), gravity=np.zeros(3, dtype), rot_diff=np.zeros((3, 3), dtype), velocity=np.zeros((F, 3), dtype),
                 Ps=np.zeros((K, 3), dtype), Rs=np.zeros((K, 3, 3), dtype), Vs=np.zeros((K, 3), dtype))
    out = dict(status=OK, pivots=np.ones(0, dtype), stages=[], fail_a0=None, flags=flags, **zeros)

    def solve(A, b, stage):
        if solver == "dense":
            return dense_solve(A, b)
        x, piv, a0 = cholesky_solve_info(A, b, T(gate))
        out["stages"].append((stage, piv))
        out["pivots"] = np.concatenate([p for _, p in out["stages"]])
        out["fail_a0"] = a0
        return x

    A, b = _system(R, Tr, tic, pre, 4, None, None)
    x = solve(A, b, "linear")
    if x is None:
        out["status"] = RANK
        return out
    s = x[-1] / T(100); g = x[-4:-1].copy()
    if not _finite(s, g):
        out["status"] = NON_FINITE
        return out
    out["scale"] = s; out["gravity_c0"] = g
    if abs(np.sqrt(g @ g) - G) > T(1) or s < 0:
        out["status"] = LINEAR
        return out
    out["linear"] = dict(scale=s, gravity_c0=g)
    g0 = normalized(g) * G
    for rnd in range(4):
        lxly = tangent_basis(g0, flags)
        A, b = _system(R, Tr, tic, pre, 3, lxly, g0)
        x = solve(A, b, "refine%d" % rnd)
        if x is None:
            out.update(status=RANK, scale=T(0), gravity_c0=np.zeros(3, dtype))
            return out
        g0 = normalized(g0 + lxly @ x[-3:-1]) * G
    g = g0
    s = x[-1] / T(100)
    if not _finite(s, g, x[:3 * F]):
        out.update(status=NON_FINITE, scale=T(0), gravity_c0=np.zeros(3, dtype))
        return out
    out.update(scale=s, gravity_c0=g, velocity=x[:3 * F].reshape(F, 3).copy())
    if s < 0:
        out["status"] = REFINED_SCALE
        return out
    # the state change
    Rs = R[key].copy()
    Ps = np.stack([s * Tr[i] - R[i] @ tic - (s * Tr[key[0]] - R[key[0]] @ tic) for i in key])
    Vs = np.stack([R[key[kv]] @ x[3 * kv:3 * kv + 3] for kv in range(K)])
    R0 = g2R(g, flags)
    yaw = r2ypr(R0 @ Rs[0])[0]
    R0 = ypr2R(np.array([-yaw, 0, 0], dtype=dtype)) @ R0
    out.update(gravity=R0 @ g, rot_diff=R0, Ps=Ps @ R0.T, Rs=np.einsum("ab,kbc->kac", R0, Rs), Vs=Vs @ R0.T)
    return out
