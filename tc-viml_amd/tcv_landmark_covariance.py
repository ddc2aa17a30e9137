"""ctypes mirror of include/tcv_landmark_covariance.h: the marginal covariance of the landmarks' inverse depths, batched on the device.

    import tcv, tcv_landmark_covariance as lc
    b = tcv.Batch(windows)
    lc.compute(b, cross=[("pose", -1), ("ex", 0)])      # variances, and the cross covariance with the newest pose and the extrinsic
    lc.variances(b, window=0)                           # one per landmark, para_feature order
    lc.cross(b, window=0, k=0)                          # landmarks x 6, tangent space
    lc.status(b)                                        # per window: 0 fine, 1 rank deficient, 2 non-finite

Its own module next to tcv_covariance.py: tcv_covariance.EXPORTS stays the list of include/tcv_covariance.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

import tcv
import tcv_covariance as cv
from tcv import TcvError, check, dptr, iptr  # noqa: F401
from tcv_covariance import KINDS, NON_FINITE, OK, RANK_DEFICIENT, SIZES, Options, default_options  # noqa: F401

MAX_CROSS = 16
EXPORTS = ["tcv_batch_compute_landmark_covariance", "tcv_batch_landmark_covariance_dims", "tcv_batch_get_landmark_variances",
           "tcv_batch_get_landmark_variances_all", "tcv_batch_get_landmark_cross", "tcv_batch_landmark_covariance_status",
           "tcv_problem_compute_landmark_covariance"]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class CrossBlock(C.Structure):
    _fields_ = [("kind", C.c_int), ("index", C.c_int)]


_bound = False


def lib():
    global _bound
    L = cv.lib()
    if not _bound:
        vp = C.c_void_p
        L.tcv_batch_compute_landmark_covariance.argtypes = [vp, C.POINTER(Options), C.POINTER(CrossBlock), C.c_int, vp]
        L.tcv_batch_landmark_covariance_dims.argtypes = [vp, C.c_int, _ip]
        L.tcv_batch_get_landmark_variances.argtypes = [vp, C.c_int, _dp, C.c_int, _ip]
        L.tcv_batch_get_landmark_variances_all.argtypes = [vp, _dp, C.c_int, _ip]
        L.tcv_batch_get_landmark_cross.argtypes = [vp, C.c_int, C.c_int, _dp, C.c_int, _ip, _ip]
        L.tcv_batch_landmark_covariance_status.argtypes = [vp, _ip, C.c_int]
        L.tcv_problem_compute_landmark_covariance.argtypes = [vp, C.POINTER(Options), C.POINTER(_dp), C.c_int, C.POINTER(CrossBlock), C.c_int, _dp,
                                                              C.POINTER(_dp), _ip]
        _bound = True
    return L


def cross_blocks(cross):
    """C array of cross blocks: (kind, index) each, kind a name of KINDS or the enum value"""
    out = [CrossBlock(KINDS[k] if isinstance(k, str) else int(k), int(i)) for k, i in cross]
    return (CrossBlock * max(1, len(out)))(*out), len(out)


def compute(batch, cross=(), at_solution=False, apply_loss_function=True, min_relative_pivot=None, stream=None):
    """tcv_batch_compute_landmark_covariance on a tcv.Batch: asynchronous on `stream`; read with variances / variances_all / cross / status"""
    o = default_options(at_solution=int(at_solution), apply_loss_function=int(apply_loss_function))
    if min_relative_pivot is not None:
        o.min_relative_pivot = float(min_relative_pivot)
    arr, n = cross_blocks(cross)
    check(lib().tcv_batch_compute_landmark_covariance(batch.h, C.byref(o), arr, n, stream))


def n_landmarks(batch, window):
    n = C.c_int()
    check(lib().tcv_batch_landmark_covariance_dims(batch.h, int(window), C.byref(n)))
    return n.value


def variances(batch, window):
    L = n_landmarks(batch, window)
    out = np.zeros(max(1, L))
    n = C.c_int()
    check(lib().tcv_batch_get_landmark_variances(batch.h, int(window), dptr(out), len(out), C.byref(n)))
    return out[:n.value].copy()


def variances_all(batch):
    """n_windows x stride (the batch's largest landmark count), the tail of a shorter window zero"""
    nw = len(batch.windows)
    stride = max([n_landmarks(batch, w) for w in range(nw)] + [1])
    out = np.zeros(nw * stride)
    s = C.c_int()
    check(lib().tcv_batch_get_landmark_variances_all(batch.h, dptr(out), len(out), C.byref(s)))
    return out[:nw * s.value].reshape(nw, s.value).copy()


def cross(batch, window, k):
    L = n_landmarks(batch, window)
    out = np.zeros(max(1, L) * 9)
    r, c = C.c_int(), C.c_int()
    check(lib().tcv_batch_get_landmark_cross(batch.h, int(window), int(k), dptr(out), len(out), C.byref(r), C.byref(c)))
    return out[:r.value * c.value].reshape(r.value, c.value).copy()


def status(batch):
    out = np.zeros(len(batch.windows), np.int32)
    check(lib().tcv_batch_landmark_covariance_status(batch.h, iptr(out), len(out)))
    return out


def problem_raw(window, addresses, cross=(), options=None, var=None, outs=None):
    """(return code, variances, cross rows, status) of tcv_problem_compute_landmark_covariance on a tcv.Window; nothing raised.
    addresses: the inverse-depth addresses (integers); var / outs: the caller's output arrays"""
    arr, nc = cross_blocks(cross)
    o = default_options() if options is None else options
    n = len(addresses)
    ads = (_dp * max(1, n))(*[C.cast(C.c_void_p(int(a)), _dp) for a in addresses])
    if var is None:
        var = np.zeros(max(1, n))
    if outs is None:
        outs = [np.zeros((max(1, n), SIZES.get(arr[k].kind, 9))) for k in range(nc)]
    ptrs = (_dp * max(1, nc))(*[dptr(a) for a in outs])
    st = C.c_int(-1)
    rc = lib().tcv_problem_compute_landmark_covariance(window.h, C.byref(o), ads, n, arr, nc, dptr(var), ptrs, C.byref(st))
    return rc, var, outs, st.value


def problem(window, landmarks=None, cross=(), **kw):
    """variances and cross rows of landmarks (indices into the window's lam array; default: all) of one tcv.Window at its current states:
    (variances, list of cross arrays, status)"""
    lam = window.lam
    idx = range(lam.shape[0]) if landmarks is None else landmarks
    base = lam.ctypes.data
    rc, var, outs, st = problem_raw(window, [base + 8 * int(l) for l in idx], cross, default_options(**kw))
    check(rc)
    return var, outs, st
