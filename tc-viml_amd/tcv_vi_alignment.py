"""ctypes mirror of include/tcv_vi_alignment.h: the batched visual-inertial alignment (VisualIMUAlignment and the state change of
Estimator::visualInitialAlign of the reference).

    import tcv_vi_alignment as va
    res = va.align([dict(R=..., T=..., tic=..., imu=[(acc0, gyr0, samples7), ...], ba0=..., bg0=..., noise=..., key_frame=[...]), ...])
    res[0]["status"], res[0]["scale"], res[0]["gravity"], res[0]["Ps"], res[0]["Rs"], res[0]["Vs"], res[0]["bg"]

Its own module next to tcv.py: tcv.EXPORTS stays the list of include/tcv.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

import tcv
from tcv import ImuPreintegration, TcvError, check, dptr, f64, i32, iptr  # noqa: F401

MAX_FRAMES, MAX_BATCH = 128, 4096
OK, LINEAR, REFINED_SCALE, RANK, NON_FINITE = 0, 1, 2, 3, 4
EXPORTS = ["tcv_vi_align_options_default", "tcv_vi_align", "tcv_vi_align_last_timing"]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Desc(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("R", _dp), ("T", _dp), ("tic", C.c_double * 3), ("first", _ip), ("count", _ip), ("samples7", _dp),
                ("num_samples", C.c_int), ("acc0_gyr0", _dp), ("ba0", C.c_double * 3), ("bg0", C.c_double * 3), ("noise", C.c_double * 4),
                ("n_key", C.c_int), ("key_frame", _ip)]


class Options(C.Structure):
    _fields_ = [("gravity_norm", C.c_double), ("min_relative_pivot", C.c_double)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("delta_bg", C.c_double * 3), ("bg", C.c_double * 3), ("scale", C.c_double), ("gravity_c0", C.c_double * 3),
                ("gravity", C.c_double * 3), ("rot_diff", C.c_double * 9), ("min_pivot", C.c_double), ("velocity", _dp), ("Ps", _dp), ("Rs", _dp),
                ("Vs", _dp), ("preint", C.POINTER(ImuPreintegration))]


_bound = False


def lib():
    global _bound
    L = tcv.lib()
    if not _bound:
        L.tcv_vi_align_options_default.argtypes = [C.POINTER(Options)]
        L.tcv_vi_align_options_default.restype = None
        L.tcv_vi_align.argtypes = [C.c_int, C.POINTER(Desc), C.POINTER(Options), C.POINTER(Result), C.c_void_p]
        L.tcv_vi_align_last_timing.argtypes = [_dp]
        _bound = True
    return L


def default_options(**kw) -> Options:
    o = Options()
    lib().tcv_vi_align_options_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class Sequence:
    """One sequence: dict(R (F x 3 x 3), T (F x 3), tic (3), imu = F - 1 tuples (acc0 (3), gyr0 (3), samples (count x 7: dt, acc, gyr)),
    ba0, bg0 (3, default 0), noise (4), key_frame (ascending indices, default all frames)).  Keeps the arrays alive behind the descriptor."""

    def __init__(self, s):
        self.R = f64(s["R"]).reshape(-1, 9)
        self.T = f64(s["T"]).reshape(-1, 3)
        self.F = self.R.shape[0]
        imu = list(s["imu"])
        self.count = i32([len(np.asarray(m[2]).reshape(-1, 7)) for m in imu])
        self.first = i32(np.concatenate([[0], np.cumsum(self.count)[:-1]])) if len(imu) else i32([])
        self.samples = f64(np.concatenate([np.asarray(m[2], dtype=np.float64).reshape(-1, 7) for m in imu])) if len(imu) else np.zeros((0, 7))
        self.init = f64([np.concatenate([np.asarray(m[0], dtype=np.float64), np.asarray(m[1], dtype=np.float64)]) for m in imu]).reshape(-1, 6)
        key = s.get("key_frame")
        self.key = i32(np.arange(self.F) if key is None else key)
        self.desc = Desc(self.F, dptr(self.R), dptr(self.T), (C.c_double * 3)(*f64(s["tic"])), iptr(self.first), iptr(self.count), dptr(self.samples),
                         len(self.samples), dptr(self.init), (C.c_double * 3)(*f64(s.get("ba0", np.zeros(3)))), (C.c_double * 3)(*f64(s.get("bg0", np.zeros(3)))),
                         (C.c_double * 4)(*f64(s["noise"])), len(self.key), iptr(self.key))


class Outputs:
    """the caller's arrays behind one tcv_vi_align_result"""

    def __init__(self, F, K, want_preint):
        self.velocity = np.zeros((max(F, 0), 3)); self.Ps = np.zeros((max(K, 0), 3)); self.Rs = np.zeros((max(K, 0), 3, 3)); self.Vs = np.zeros((max(K, 0), 3))
        self.preint = (ImuPreintegration * max(F - 1, 1))() if want_preint else None

    def bind(self, r: Result):
        r.velocity, r.Ps, r.Rs, r.Vs = dptr(self.velocity), dptr(self.Ps), dptr(self.Rs), dptr(self.Vs)
        r.preint = self.preint if self.preint is not None else None


def align_raw(descs, options=None, stream=None, want_preint=False):
    """(status, results, outputs) of tcv_vi_align over a list of Desc; nothing raised"""
    n = len(descs)
    arr = (Desc * max(n, 1))(*descs)
    res = (Result * max(n, 1))()
    outs = [Outputs(d.n_frames, d.n_key, want_preint) for d in descs]
    for k, o in enumerate(outs):
        o.bind(res[k])
    rc = lib().tcv_vi_align(n, arr, C.byref(options) if options is not None else None, res, stream)
    return rc, res, outs


def preint_dict(arr, n) -> dict:
    return dict(delta_p=np.array([list(arr[i].delta_p) for i in range(n)]), delta_q=np.array([list(arr[i].delta_q) for i in range(n)]),
                delta_v=np.array([list(arr[i].delta_v) for i in range(n)]), lin_ba=np.array([list(arr[i].linearized_ba) for i in range(n)]),
                lin_bg=np.array([list(arr[i].linearized_bg) for i in range(n)]), sum_dt=np.array([arr[i].sum_dt for i in range(n)]),
                jacobian=np.array([list(arr[i].jacobian) for i in range(n)]).reshape(n, 15, 15),
                covariance=np.array([list(arr[i].covariance) for i in range(n)]).reshape(n, 15, 15))


def align(sequences, options=None, stream=None, want_preint=False):
    """One device batch over a list of sequence dicts (or Sequence objects); a list of dicts, one per sequence"""
    S = [s if isinstance(s, Sequence) else Sequence(s) for s in sequences]
    rc, res, outs = align_raw([s.desc for s in S], options, stream, want_preint)
    check(rc)
    out = []
    for k, s in enumerate(S):
        r, o = res[k], outs[k]
        d = dict(status=int(r.status), delta_bg=np.array(r.delta_bg[:]), bg=np.array(r.bg[:]), scale=float(r.scale), gravity_c0=np.array(r.gravity_c0[:]),
                 gravity=np.array(r.gravity[:]), rot_diff=np.array(r.rot_diff[:]).reshape(3, 3), min_pivot=float(r.min_pivot), velocity=o.velocity,
                 Ps=o.Ps, Rs=o.Rs, Vs=o.Vs)
        if want_preint:
            d["preint"] = preint_dict(o.preint, s.F - 1)
        out.append(d)
    return out


def last_timing():
    out = np.zeros(8)
    check(lib().tcv_vi_align_last_timing(dptr(out)))
    return dict(pack_ms=out[0], preint1_ms=out[1], bias_ms=out[2], preint2_ms=out[3], align_ms=out[4], bias_kernel_ms=out[5], align_kernel_ms=out[6])
