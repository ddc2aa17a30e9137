"""Test helper for the batched marginal covariance (include/tcv_covariance.h): the yardstick the device is measured with, and what a
float64 implementation of the same mathematics can reach.

The reduced camera system S of a window has a condition number around 1e15 (5e11 after symmetric diagonal scaling), so a float64
Cholesky inverse of a float64 S is off by 1e-6 .. 1e-4 relative and cannot be the reference.  The yardstick: J in float64 from
np_oracle.Problem.linearize, S = H_cc - sum_l h_l h_l' / H_ll assembled in np.longdouble (64-bit mantissa), its inverse refined in
np.longdouble from a float64 Cholesky start with X <- X + X (I - S X) until |I - S X| stalls, on the diagonally scaled system.  `mp_inverse`
(50 digits, mpmath) cross-checks it on small windows.

Error measure over blocks: e(C) = max_ij |C_ij - Cx_ij| / sqrt(Cx_ii Cx_jj) -- invariant under the scaling of the unknowns."""
import numpy as np
import scipy.linalg

import np_oracle as NO

LD = np.longdouble


def linearize(w, x=None, ex_constant=False):
    """(problem, J, x): the oracle's float64 Jacobian of the window at x (default: its own states)"""
    P = NO.Problem(w, ex_constant=ex_constant)
    x = P.x0() if x is None else x
    J, r, cost = P.linearize(x)
    return P, J, x


def normal_matrix_ld(J):
    """H = J'J in np.longdouble, row by row over each row's non-zero columns"""
    n = J.shape[1]
    H = np.zeros((n, n), LD)
    for row in J:
        ix = np.nonzero(row)[0]
        v = row[ix].astype(LD)
        H[np.ix_(ix, ix)] += np.outer(v, v)
    return H


def schur(H, nc):
    """S = H_cc - H_cl diag(H_ll)^-1 H_lc in the dtype of H; asserts that H_ll is diagonal"""
    Hll = H[nc:, nc:]
    d = np.diag(Hll).copy()
    assert np.abs(Hll - np.diag(d)).max(initial=0) == 0, "H_ll is not diagonal"
    Hcl = H[:nc, nc:]
    keep = d > 0
    return H[:nc, :nc] - (Hcl[:, keep] / d[keep]) @ Hcl[:, keep].T


def reduced_system_ld(P, J):
    return schur(normal_matrix_ld(J), P.nc)


def reduced_system_f64(P, J, order=0):
    """the float64 S in one of two summation orders: 0 = BLAS J'J, 1 = the rows accumulated one by one from the last to the first"""
    if order == 0:
        H = J.T @ J
    else:
        H = np.zeros((J.shape[1], J.shape[1]))
        for row in J[::-1]:
            ix = np.nonzero(row)[0]
            H[np.ix_(ix, ix)] += np.outer(row[ix], row[ix])
    return schur(H, P.nc)


def inverse_ld(S, max_iter=12):
    """(X, history of |I - S X|_max on the scaled system): S^-1 in np.longdouble"""
    S = np.asarray(S, LD)
    d = 1 / np.sqrt(np.diag(S))
    Ss = S * d[:, None] * d[None, :]
    c = scipy.linalg.cho_factor(Ss.astype(float), lower=True)
    X = scipy.linalg.cho_solve(c, np.eye(len(S))).astype(LD)
    I = np.eye(len(S), dtype=LD)
    hist, best, bestX = [], np.inf, X
    for _ in range(max_iter):
        R = I - Ss @ X
        r = float(np.abs(R).max())
        hist.append(r)
        if r >= 0.5 * best and len(hist) > 1:      # stalled
            if r < best:
                bestX = X
            break
        best, bestX = r, X
        X = X + X @ R
    return bestX * d[:, None] * d[None, :], hist


def mp_inverse(S, digits=50):
    """S^-1 at `digits` digits (mpmath), returned in np.longdouble"""
    import mpmath
    n = len(S)
    with mpmath.workdps(digits):
        M = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mpmath.mpf(float(S[i, j])) + mpmath.mpf(float(S[i, j] - LD(float(S[i, j]))))      # both halves of the long double
        X = M ** -1
        out = np.zeros((n, n), LD)
        for i in range(n):
            for j in range(n):
                hi = float(X[i, j])
                out[i, j] = LD(hi) + LD(float(X[i, j] - mpmath.mpf(hi)))
    return out


def e_full(C, Cx):
    """e over the whole matrix"""
    Cx = np.asarray(Cx, LD)
    s = np.sqrt(np.diag(Cx))
    return float((np.abs(np.asarray(C, LD) - Cx) / np.outer(s, s)).max())


def e_block(C, Cx, ri, rj):
    """e of one block: C the block, Cx the full reference, ri / rj the index ranges of its rows / columns"""
    Cx = np.asarray(Cx, LD)
    s = np.sqrt(np.diag(Cx))
    ref = Cx[np.ix_(ri, rj)]
    return float((np.abs(np.asarray(C, LD) - ref) / np.outer(s[ri], s[rj])).max())


def f64_inverse(S):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(np.asarray(S, float), lower=True), np.eye(len(S)))


def relative_pivots(S):
    """L_kk^2 / S_kk of a float64 Cholesky factorisation that does not stop at a failing pivot: (array up to the first pivot <= 0, that
    pivot or None)"""
    A = np.array(S, float)
    n = len(A)
    d0 = np.diag(A).copy()
    out = []
    for k in range(n):
        d = A[k, k]
        if not d > 0:
            return np.array(out), d / d0[k]
        out.append(d / d0[k])
        A[k + 1:, k] /= np.sqrt(d)
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return np.array(out), None


def block_range(P, kind, index):
    """tangent index range of a camera-side block of an np_oracle.Problem (negative frame indices count from the newest); None: constant"""
    if kind in ("pose", "sb") and index < 0:
        index += P.F
    lo = P.loff[(kind, index)]
    if lo < 0:
        return None
    return np.arange(lo, lo + {"pose": 6, "sb": 9, "ex": 6, "td": 1, "relo": 6}[kind])


class Reference:
    """Everything the tests need of one window, computed once: the yardstick Cx, and the error of the float64 path in two orders"""

    def __init__(self, w, x=None, ex_constant=False):
        self.P, self.J, self.x = linearize(w, x, ex_constant)
        self.S = reduced_system_ld(self.P, self.J)
        self.Cx, self.hist = inverse_ld(self.S)
        self.C64 = [f64_inverse(reduced_system_f64(self.P, self.J, o)) for o in (0, 1)]
        self.e_f64 = [e_full(C, self.Cx) for C in self.C64]

    def block(self, bi, bj):
        ri, rj = block_range(self.P, *bi), block_range(self.P, *bj)
        if ri is None or rj is None:
            return None
        return np.asarray(self.Cx[np.ix_(ri, rj)], float)

    def e_f64_block(self, bi, bj):
        """the float64 path's error on one block, the larger of the two orders"""
        ri, rj = block_range(self.P, *bi), block_range(self.P, *bj)
        if ri is None or rj is None:
            return 0.0
        return max(e_block(C[np.ix_(ri, rj)], self.Cx, ri, rj) for C in self.C64)

    def e(self, C, bi, bj):
        ri, rj = block_range(self.P, *bi), block_range(self.P, *bj)
        if ri is None or rj is None:
            return 0.0 if not np.any(C) else float("inf")
        return e_block(C, self.Cx, ri, rj)
