"""ctypes mirror of include/tcv_pose_graph.h: the batched 4-DoF pose-graph optimisation (PoseGraph::optimize4DoF of the reference).

    import tcv_pose_graph as pg
    res = pg.optimize([dict(t=..., q=..., sequence=..., loops=[(cur, old, relative_t, relative_yaw), ...]), ...])
    res[0]["t"], res[0]["R"], res[0]["summary"]

Its own module next to tcv.py: tcv.EXPORTS stays the list of include/tcv.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

import tcv
from tcv import TcvError, check, dptr, f64, i32, iptr  # noqa: F401

MAX_NODES, MAX_LOOPS, MAX_BATCH, MAX_TRACE = 2048, 256, 4096, 16
EXPORTS = ["tcv_pose_graph_options_default", "tcv_pose_graphs_optimize", "tcv_pose_graph_eval_edges", "tcv_pose_graph_plan_stats",
           "tcv_pose_graph_last_timing"]
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Desc(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("t", _dp), ("q_xyzw", _dp), ("sequence", _ip), ("n_loops", C.c_int), ("loop_cur", _ip), ("loop_old", _ip),
                ("loop_relative_t", _dp), ("loop_relative_yaw", _dp)]


class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("huber_delta", C.c_double), ("loop_weight", C.c_double), ("loop_yaw_divisor", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("termination", C.c_int), ("num_free_nodes", C.c_int), ("num_edges", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("cost", C.c_double * MAX_TRACE), ("cost_candidate", C.c_double * MAX_TRACE), ("rho", C.c_double * MAX_TRACE), ("radius", C.c_double * MAX_TRACE),
                ("step", C.c_int * MAX_TRACE), ("yaw_drift", C.c_double), ("r_drift", C.c_double * 9), ("t_drift", C.c_double * 3)]


_bound = False


def lib():
    global _bound
    L = tcv.lib()
    if not _bound:
        L.tcv_pose_graph_options_default.argtypes = [C.POINTER(Options)]
        L.tcv_pose_graph_options_default.restype = None
        L.tcv_pose_graphs_optimize.argtypes = [C.c_int, C.POINTER(Desc), C.POINTER(Options), C.POINTER(_dp), C.POINTER(_dp), C.POINTER(Summary), C.c_void_p]
        L.tcv_pose_graph_eval_edges.argtypes = [C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.POINTER(Options), _dp, _dp, _dp]
        L.tcv_pose_graph_plan_stats.argtypes = [C.POINTER(Desc), C.POINTER(C.c_longlong), _ip]
        L.tcv_pose_graph_last_timing.argtypes = [_dp]
        _bound = True
    return L


def default_options(**kw) -> Options:
    o = Options()
    lib().tcv_pose_graph_options_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class Graph:
    """One graph: dict(t (n x 3), q (n x 4, xyzw), sequence (n ints or None), loops [(cur, old, relative_t (3), relative_yaw)]).  Keeps the
    arrays alive behind the descriptor."""

    def __init__(self, g):
        self.t = f64(g["t"]).reshape(-1, 3)
        self.q = f64(g["q"]).reshape(-1, 4)
        self.n = self.t.shape[0]
        seq = g.get("sequence")
        self.seq = None if seq is None else i32(seq)
        loops = list(g.get("loops", []))
        self.cur = i32([l[0] for l in loops]); self.old = i32([l[1] for l in loops])
        self.rel_t = f64([l[2] for l in loops]).reshape(-1, 3); self.rel_yaw = f64([l[3] for l in loops])
        self.desc = Desc(self.n, dptr(self.t), dptr(self.q), None if self.seq is None else iptr(self.seq), len(loops),
                         iptr(self.cur) if loops else None, iptr(self.old) if loops else None, dptr(self.rel_t) if loops else None,
                         dptr(self.rel_yaw) if loops else None)


def summary_dict(s: Summary) -> dict:
    k = min(s.iterations, MAX_TRACE)
    return dict(iterations=s.iterations, termination=s.termination, num_free_nodes=s.num_free_nodes, num_edges=s.num_edges,
                initial_cost=s.initial_cost, final_cost=s.final_cost, cost=np.array(s.cost[:k]), cost_candidate=np.array(s.cost_candidate[:k]),
                rho=np.array(s.rho[:k]), radius=np.array(s.radius[:k]), step=[int(v) for v in s.step[:k]], yaw_drift=s.yaw_drift,
                r_drift=np.array(s.r_drift[:]).reshape(3, 3), t_drift=np.array(s.t_drift[:]))


def optimize_raw(descs, options=None, stream=None):
    """(status, t list, R list, summaries) of tcv_pose_graphs_optimize over a list of Desc; nothing raised"""
    n = len(descs)
    arr = (Desc * max(n, 1))(*descs)
    t_out = [np.zeros((max(d.n_nodes, 0), 3)) for d in descs]
    R_out = [np.zeros((max(d.n_nodes, 0), 3, 3)) for d in descs]
    tp = (_dp * max(n, 1))(*[dptr(a) for a in t_out]); Rp = (_dp * max(n, 1))(*[dptr(a) for a in R_out])
    sums = (Summary * max(n, 1))()
    rc = lib().tcv_pose_graphs_optimize(n, arr, C.byref(options) if options is not None else None, tp, Rp, sums, stream)
    return rc, t_out, R_out, sums


def optimize(graphs, options=None, stream=None):
    """One device batch over a list of graph dicts (or Graph objects); a list of dict(t, R, summary)"""
    G = [g if isinstance(g, Graph) else Graph(g) for g in graphs]
    rc, t_out, R_out, sums = optimize_raw([g.desc for g in G], options, stream)
    check(rc)
    return [dict(t=t_out[k], R=R_out[k], summary=summary_dict(sums[k])) for k in range(len(G))]


def eval_edges(kind, yaw_i, t_i, yaw_j, t_j, meas, options=None):
    """residual (n x 4), jacobian (n x 2 x 4 x 4), cost (n) of n independent edges on the device"""
    kind = i32(kind); n = len(kind)
    yaw_i, t_i, yaw_j, t_j, meas = f64(yaw_i), f64(t_i).reshape(-1, 3), f64(yaw_j), f64(t_j).reshape(-1, 3), f64(meas).reshape(-1, 6)
    r = np.zeros((n, 4)); J = np.zeros((n, 2, 4, 4)); c = np.zeros(n)
    check(lib().tcv_pose_graph_eval_edges(n, iptr(kind), dptr(yaw_i), dptr(t_i), dptr(yaw_j), dptr(t_j), dptr(meas),
                                          C.byref(options) if options is not None else None, dptr(r), dptr(J), dptr(c)))
    return r, J, c


def plan_stats(graph):
    """the host-side elimination order of one graph: dict(free, band, border, edges, fixed_edges, half_bandwidth, scratch_bytes, position)"""
    g = graph if isinstance(graph, Graph) else Graph(graph)
    out = (C.c_longlong * 8)()
    pos = np.zeros(max(g.n, 1), np.int32)
    check(lib().tcv_pose_graph_plan_stats(C.byref(g.desc), out, iptr(pos)))
    return dict(free=int(out[0]), band=int(out[1]), border=int(out[2]), edges=int(out[3]), fixed_edges=int(out[4]), half_bandwidth=int(out[5]),
                scratch_bytes=int(out[6]), position=pos[:g.n].copy())


def last_timing():
    out = np.zeros(4)
    check(lib().tcv_pose_graph_last_timing(dptr(out)))
    return dict(pack_ms=out[0], upload_ms=out[1], kernel_ms=out[2], download_ms=out[3])
