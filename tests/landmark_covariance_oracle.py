"""Test helper for the landmarks' marginal covariance (include/tcv_landmark_covariance.h): the yardstick and the float64 path.

With H = J'J of a window (camera-side tangent space c first, then one column per landmark), Cx = S^-1 the long-double yardstick of
tests/covariance_oracle.py, h_l = H_cl and w_l = h_l / H_ll:

    var(lambda_l)           = 1 / H_ll + w_l' Cx w_l
    cov(lambda_l, column j) = -(Cx w_l)_j

all in np.longdouble, H from covariance_oracle.normal_matrix_ld.  The float64 path is the same formula in float64 with the float64
inverses Reference.C64, in their two summation orders.  An independent route -- the landmark rows of a long-double inverse of the FULL
H, camera side and landmarks together -- says how far the yardstick itself can be trusted.

Error measures, of the form of covariance_oracle's e: variances |v - vx| / vx; cross entries |c - cx| / sqrt(vx_l Cx_jj)."""
import numpy as np

import covariance_cases as CC
import covariance_oracle as CO

LD = CO.LD

PARITY_CASES = ("frames4", "frames6_td", "full", "constant_extrinsic", "relocalisation", "golden_prior", "landmarks200")


def cross_list(w):
    """the cross blocks of a window: newest pose, newest speed-bias, extrinsic, pose 0, plus td or the relocalisation pose where it has one"""
    cr = [("pose", -1), ("sb", -1), ("ex", 0), ("pose", 0)]
    if w.get("td") is not None:
        cr.append(("td", 0))
    if w.get("relo") is not None:
        cr.append(("relo", 0))
    return cr


def features_in_registration_order(w):
    """True when the window's point factors name the landmarks 0, 1, 2, ... in order of first appearance and leave none out: then the
    problem's l-th registered inverse-depth block is para_feature[l], and the oracle's landmark l is the library's"""
    lm = np.asarray(w["proj"]["landmark"], dtype=int)
    first = lm[np.sort(np.unique(lm, return_index=True)[1])]
    return len(first) == w["lam"].shape[0] and np.array_equal(first, np.arange(len(first)))


def normal_matrix_f64(J, order):
    """H = J'J in float64 in the two summation orders of covariance_oracle.reduced_system_f64"""
    if order == 0:
        return J.T @ J
    H = np.zeros((J.shape[1], J.shape[1]))
    for row in J[::-1]:
        ix = np.nonzero(row)[0]
        H[np.ix_(ix, ix)] += np.outer(row[ix], row[ix])
    return H


def landmark_rows(H, C, nc):
    """(variances, cross rows L x nc) of the formula, in the dtype of H and C; a landmark without information (H_ll = 0) gives zeros"""
    d = np.diag(H)[nc:].copy()
    keep = d > 0
    inv = np.zeros_like(d)
    inv[keep] = 1 / d[keep]
    w = H[:nc, nc:] * inv[None, :]
    Cw = C @ w
    return inv + (w * Cw).sum(axis=0), -Cw.T


def e_var(v, vx):
    vx = np.asarray(vx, LD)
    return float((np.abs(np.asarray(v, LD) - vx) / vx).max())


def e_cross(c, cx, vx, cjj):
    """c, cx: L x width; vx: the L reference variances; cjj: the reference variances of the block's columns"""
    if c.size == 0:
        return 0.0
    s = np.sqrt(np.outer(np.asarray(vx, LD), np.asarray(cjj, LD)))
    return float((np.abs(np.asarray(c, LD) - np.asarray(cx, LD)) / s).max())


class LandmarkReference:
    """Everything the tests need of one window, computed once from its covariance_oracle.Reference: the yardstick's variances and cross
    rows, and the same from the float64 path in its two orders"""

    def __init__(self, ref):
        self.ref, self.P = ref, ref.P
        nc = ref.P.nc
        self.H = CO.normal_matrix_ld(ref.J)
        self.var, self.rows = landmark_rows(self.H, np.asarray(ref.Cx, LD), nc)
        self.cdiag = np.diag(np.asarray(ref.Cx, LD))
        self.f64 = [landmark_rows(normal_matrix_f64(ref.J, o), ref.C64[o], nc) for o in (0, 1)]
        self.hll64 = np.diag(normal_matrix_f64(ref.J, 0))[nc:].copy()

    def columns(self, block):
        """tangent index range of a cross block; None: constant in this window"""
        return CO.block_range(self.P, *block)

    def cross(self, block):
        r = self.columns(block)
        return None if r is None else np.asarray(self.rows[:, r], float)

    def e_var(self, v):
        return e_var(v, self.var)

    def e_cross(self, c, block):
        r = self.columns(block)
        if r is None:
            return 0.0 if not np.any(c) else float("inf")
        return e_cross(c, self.rows[:, r], self.var, self.cdiag[r])

    def e_var_f64(self):
        return max(e_var(v, self.var) for v, _ in self.f64)

    def e_cross_f64(self, block):
        r = self.columns(block)
        if r is None:
            return 0.0
        return max(e_cross(rows[:, r], self.rows[:, r], self.var, self.cdiag[r]) for _, rows in self.f64)


def full_inverse_rows(lref):
    """the independent route: (variances, cross rows L x nc) read off a long-double inverse of the FULL H"""
    nc = lref.P.nc
    X, hist = CO.inverse_ld(lref.H)
    return np.diag(X)[nc:].copy(), X[nc:, :nc].copy()


_REF = {}


def reference(name, x=None, loss=True, key=None):
    """LandmarkReference of a case of covariance_cases, cached like covariance_cases.reference (and built on it)"""
    k = (name, loss, key)
    if k not in _REF:
        _REF[k] = LandmarkReference(CC.reference(name, x, loss, key))
    return _REF[k]
