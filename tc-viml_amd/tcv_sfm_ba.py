"""ctypes mirror of include/tcv_sfm_ba.h: the batched bundle adjustment of the initial SfM (the full BA of GlobalSFM::construct of the reference).

    import tcv_sfm_ba as ba
    res = ba.bundle_adjust([dict(c_rotation=..., c_translation=..., l=..., position=..., observations=[[(frame, u, v), ...] per point]), ...])
    res[0]["c_rotation"], res[0]["c_translation"], res[0]["position"], res[0]["q"], res[0]["T"], res[0]["summary"]

Its own module next to tcv.py: tcv.EXPORTS stays the list of include/tcv.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

import tcv
from tcv import TcvError, check, dptr, f64, i32, iptr  # noqa: F401

MAX_FRAMES, MAX_POINTS, MAX_BATCH, MAX_TRACE = 15, 1024, 4096, 64
EXPORTS = ["tcv_sfm_ba", "tcv_sfm_ba_options_default", "tcv_sfm_ba_eval_observations", "tcv_sfm_ba_plan_stats", "tcv_sfm_ba_last_timing"]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Desc(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("l", C.c_int), ("c_rotation", _dp), ("c_translation", _dp), ("n_points", C.c_int), ("position", _dp),
                ("obs_first", _ip), ("obs_count", _ip), ("n_obs", C.c_int), ("obs_frame", _ip), ("obs_uv", _dp)]


class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("max_num_consecutive_invalid_steps", C.c_int), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("accept_cost", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("termination", C.c_int), ("accepted", C.c_int), ("num_camera_unknowns", C.c_int), ("num_points", C.c_int),
                ("num_observations", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("cost", C.c_double * MAX_TRACE), ("cost_candidate", C.c_double * MAX_TRACE), ("rho", C.c_double * MAX_TRACE), ("radius", C.c_double * MAX_TRACE),
                ("step", C.c_int * MAX_TRACE)]


class Result(C.Structure):
    _fields_ = [("c_rotation", _dp), ("c_translation", _dp), ("position", _dp), ("q", _dp), ("T", _dp), ("summary", Summary)]


_bound = False


def lib():
    global _bound
    L = tcv.lib()
    if not _bound:
        L.tcv_sfm_ba_options_default.argtypes = [C.POINTER(Options)]
        L.tcv_sfm_ba_options_default.restype = None
        L.tcv_sfm_ba.argtypes = [C.c_int, C.POINTER(Desc), C.POINTER(Options), C.POINTER(Result), C.c_void_p]
        L.tcv_sfm_ba_eval_observations.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        L.tcv_sfm_ba_plan_stats.argtypes = [C.POINTER(Desc), C.POINTER(C.c_longlong)]
        L.tcv_sfm_ba_last_timing.argtypes = [_dp]
        _bound = True
    return L


def default_options(**kw) -> Options:
    o = Options()
    lib().tcv_sfm_ba_options_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class Problem:
    """One problem: dict(c_rotation (F x 4, w x y z), c_translation (F x 3), l, position (P x 3), observations: per point a list of
    (frame, u, v)).  Keeps the arrays alive behind the descriptor."""

    def __init__(self, p):
        self.rot = f64(p["c_rotation"]).reshape(-1, 4).copy()
        self.tr = f64(p["c_translation"]).reshape(-1, 3).copy()
        self.pos = f64(p["position"]).reshape(-1, 3).copy()
        obs = p["observations"]
        self.count = i32([len(o) for o in obs])
        self.first = i32(np.concatenate([[0], np.cumsum(self.count)[:-1]])) if len(obs) else i32([])
        flat = [o for po in obs for o in po]
        self.frame = i32([o[0] for o in flat])
        self.uv = f64([[o[1], o[2]] for o in flat]).reshape(-1, 2)
        self.F, self.P = self.rot.shape[0], self.pos.shape[0]
        self.desc = Desc(self.F, int(p["l"]), dptr(self.rot), dptr(self.tr), self.P, dptr(self.pos), iptr(self.first), iptr(self.count), len(flat),
                         iptr(self.frame), dptr(self.uv))


def summary_dict(s: Summary) -> dict:
    k = min(s.iterations, MAX_TRACE)
    return dict(iterations=s.iterations, termination=s.termination, accepted=bool(s.accepted), num_camera_unknowns=s.num_camera_unknowns,
                num_points=s.num_points, num_observations=s.num_observations, initial_cost=s.initial_cost, final_cost=s.final_cost,
                cost=np.array(s.cost[:k]), cost_candidate=np.array(s.cost_candidate[:k]), rho=np.array(s.rho[:k]), radius=np.array(s.radius[:k]),
                step=[int(v) for v in s.step[:k]])


def bundle_adjust_raw(descs, options=None, stream=None, world_frame=True):
    """(status, output arrays per problem, Result array) of tcv_sfm_ba over a list of Desc; nothing raised"""
    n = len(descs)
    out = [dict(c_rotation=np.zeros((max(d.n_frames, 0), 4)), c_translation=np.zeros((max(d.n_frames, 0), 3)), position=np.zeros((max(d.n_points, 0), 3)),
                q=np.zeros((max(d.n_frames, 0), 4)), T=np.zeros((max(d.n_frames, 0), 3))) for d in descs]
    res = (Result * max(n, 1))()
    for k, o in enumerate(out):
        res[k].c_rotation, res[k].c_translation, res[k].position = dptr(o["c_rotation"]), dptr(o["c_translation"]), dptr(o["position"])
        if world_frame:
            res[k].q, res[k].T = dptr(o["q"]), dptr(o["T"])
    arr = (Desc * max(n, 1))(*descs)
    rc = lib().tcv_sfm_ba(n, arr, C.byref(options) if options is not None else None, res, stream)
    return rc, out, res


def bundle_adjust(problems, options=None, stream=None):
    """One device batch over a list of problem dicts (or Problem objects); a list of dict(c_rotation, c_translation, position, q, T, summary)"""
    P = [p if isinstance(p, Problem) else Problem(p) for p in problems]
    rc, out, res = bundle_adjust_raw([p.desc for p in P], options, stream)
    check(rc)
    return [dict(out[k], summary=summary_dict(res[k].summary)) for k in range(len(P))]


def eval_observations(rotation, translation, point, uv):
    """residual (n x 2), jacobian (n x 2 x 9: rotation tangent 3 | translation 3 | point 3), cost (n) of n independent observations on the device"""
    rotation, translation, point, uv = f64(rotation).reshape(-1, 4), f64(translation).reshape(-1, 3), f64(point).reshape(-1, 3), f64(uv).reshape(-1, 2)
    n = rotation.shape[0]
    r = np.zeros((n, 2)); J = np.zeros((n, 2, 9)); c = np.zeros(n)
    check(lib().tcv_sfm_ba_eval_observations(n, dptr(rotation), dptr(translation), dptr(point), dptr(uv), dptr(r), dptr(J), dptr(c)))
    return r, J, c


def plan_stats(problem):
    """host only: dict(camera_unknowns, points, observations, lds_bytes, scratch_bytes, row_length, chunk_points)"""
    p = problem if isinstance(problem, Problem) else Problem(problem)
    out = (C.c_longlong * 8)()
    check(lib().tcv_sfm_ba_plan_stats(C.byref(p.desc), out))
    return dict(camera_unknowns=int(out[0]), points=int(out[1]), observations=int(out[2]), lds_bytes=int(out[3]), scratch_bytes=int(out[4]),
                row_length=int(out[5]), chunk_points=int(out[6]))


def last_timing():
    out = np.zeros(4)
    check(lib().tcv_sfm_ba_last_timing(dptr(out)))
    return dict(pack_ms=out[0], upload_ms=out[1], kernel_ms=out[2], download_ms=out[3])
