"""ctypes mirror of include/tcv_covariance.h: the batched marginal covariance of window states (ceres::Covariance on the device).

    import tcv, tcv_covariance as cv
    b = tcv.Batch(windows)
    cv.compute(b, [("pose", -1), (("pose", -1), ("sb", -1))])        # newest pose; newest pose x newest speed-bias
    cv.block(b, window=0, k=0)                                       # 6 x 6, tangent space
    cv.status(b)                                                     # per window: 0 fine, 1 rank deficient, 2 non-finite

Its own module next to tcv.py: tcv.EXPORTS stays the list of include/tcv.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

import tcv
from tcv import TcvError, check, dptr, iptr  # noqa: F401

MAX_DIM, MAX_BLOCKS = 184, 512
MIN_RELATIVE_PIVOT = 3e-13
OK, RANK_DEFICIENT, NON_FINITE = 0, 1, 2
KINDS = {"pose": 0, "sb": 1, "ex": 2, "td": 3, "relo": 4, "lam": 5}
SIZES = {0: 6, 1: 9, 2: 6, 3: 1, 4: 6}
EXPORTS = ["tcv_covariance_options_default", "tcv_batch_compute_covariance", "tcv_batch_get_covariance", "tcv_batch_get_covariance_all",
           "tcv_batch_covariance_status", "tcv_problem_compute_covariance", "tcv_covariance_pivot_status"]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Options(C.Structure):
    _fields_ = [("at_solution", C.c_int), ("apply_loss_function", C.c_int), ("min_relative_pivot", C.c_double)]


class Block(C.Structure):
    _fields_ = [("kind_i", C.c_int), ("index_i", C.c_int), ("kind_j", C.c_int), ("index_j", C.c_int)]


_bound = False


def lib():
    global _bound
    L = tcv.lib()
    if not _bound:
        vp = C.c_void_p
        L.tcv_covariance_options_default.argtypes = [C.POINTER(Options)]
        L.tcv_covariance_options_default.restype = None
        L.tcv_batch_compute_covariance.argtypes = [vp, C.POINTER(Options), C.POINTER(Block), C.c_int, vp]
        L.tcv_batch_get_covariance.argtypes = [vp, C.c_int, C.c_int, _dp, C.c_int, _ip, _ip]
        L.tcv_batch_get_covariance_all.argtypes = [vp, C.c_int, _dp, C.c_int, _ip, _ip]
        L.tcv_batch_covariance_status.argtypes = [vp, _ip, C.c_int]
        L.tcv_problem_compute_covariance.argtypes = [vp, C.POINTER(Options), C.POINTER(Block), C.c_int, C.POINTER(_dp), _ip]
        L.tcv_covariance_pivot_status.argtypes = [C.c_double, C.c_double, C.c_double]
        _bound = True
    return L


def default_options(**kw) -> Options:
    o = Options()
    lib().tcv_covariance_options_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def _half(h):
    kind, index = h
    return (KINDS[kind] if isinstance(kind, str) else int(kind)), int(index)


def blocks(requests):
    """C array of requests.  A request is (kind, index) -- the diagonal block -- or ((kind_i, index_i), (kind_j, index_j)); kind is a name
    of KINDS or the enum value"""
    out = []
    for r in requests:
        bi, bj = (r, r) if not isinstance(r[0], (tuple, list)) else r
        out.append(Block(*_half(bi), *_half(bj)))
    return (Block * max(1, len(out)))(*out), len(out)


def compute(batch, requests, at_solution=False, apply_loss_function=True, min_relative_pivot=None, stream=None):
    """tcv_batch_compute_covariance on a tcv.Batch: asynchronous on `stream`; read with block / block_all / status"""
    o = default_options(at_solution=int(at_solution), apply_loss_function=int(apply_loss_function))
    if min_relative_pivot is not None:
        o.min_relative_pivot = float(min_relative_pivot)
    arr, n = blocks(requests)
    check(lib().tcv_batch_compute_covariance(batch.h, C.byref(o), arr, n, stream))


def block(batch, window, k):
    out = np.zeros(81)
    r, c = C.c_int(), C.c_int()
    check(lib().tcv_batch_get_covariance(batch.h, int(window), int(k), dptr(out), 81, C.byref(r), C.byref(c)))
    return out[:r.value * c.value].reshape(r.value, c.value).copy()


def block_all(batch, k):
    n = len(batch.windows)
    out = np.zeros(n * 81)
    r, c = C.c_int(), C.c_int()
    check(lib().tcv_batch_get_covariance_all(batch.h, int(k), dptr(out), len(out), C.byref(r), C.byref(c)))
    return out[:n * r.value * c.value].reshape(n, r.value, c.value).copy()


def status(batch):
    out = np.zeros(len(batch.windows), np.int32)
    check(lib().tcv_batch_covariance_status(batch.h, iptr(out), len(out)))
    return out


def problem_covariance_raw(window, requests, options=None, outs=None):
    """(return code, blocks, status) of tcv_problem_compute_covariance on a tcv.Window; nothing raised.  outs: the caller's output arrays"""
    arr, n = blocks(requests)
    o = default_options() if options is None else options
    if outs is None:
        outs = [np.zeros((SIZES.get(arr[k].kind_i, 9), SIZES.get(arr[k].kind_j, 9))) for k in range(n)]
    ptrs = (_dp * max(1, n))(*[dptr(a) for a in outs])
    st = C.c_int(-1)
    rc = lib().tcv_problem_compute_covariance(window.h, C.byref(o), arr, n, ptrs, C.byref(st))
    return rc, outs, st.value


def problem_covariance(window, requests, **kw):
    """the requested blocks of one tcv.Window at its current states: (list of arrays, status)"""
    rc, outs, st = problem_covariance_raw(window, requests, default_options(**kw))
    check(rc)
    return outs, st
