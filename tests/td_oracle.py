"""Helpers of tests/test_gpu_estimator_td.py: a native lock-step replay with the window tap on (both snapshots of every window), the oracle
window rebuilt from them, and the NumPy restatement's solve of such windows on worker processes (oracle/np_oracle.py takes seconds per window;
the workers never touch the device)."""
import ctypes as C
import os
import sys

import numpy as np

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Snapshot(C.Structure):      # tcv_window_snapshot (include/tcv_estimator.h)
    _fields_ = [(k, C.c_int) for k in ("n_frames", "n_landmarks", "n_imu", "n_proj", "n_line", "marg_flag", "estimate_extrinsic", "line_exact_jacobian")] + \
               [(k, _dp) for k in ("pose_in", "speedbias_in", "ex_pose_in", "feature_in", "pose_out", "speedbias_out", "ex_pose_out", "feature_out")] + \
               [("imu", C.c_void_p), ("imu_frame_i", _ip), ("imu_frame_j", _ip), ("proj_frame_i", _ip), ("proj_frame_j", _ip), ("proj_feature", _ip), ("proj_pts", _dp),
                ("line_frame", _ip), ("line_data", _dp), ("line_K", C.c_double * 9), ("line_Ric", C.c_double * 9), ("line_Tic", C.c_double * 3), ("gravity", C.c_double * 3),
                ("proj_sqrt_info", C.c_double), ("prior_m", C.c_int), ("prior_n", C.c_int), ("prior_nblk", C.c_int),
                ("prior_block_kind", _ip), ("prior_block_index", _ip), ("prior_block_size", _ip), ("prior_block_idx", _ip),
                ("prior_x0", _dp), ("prior_J0", _dp), ("prior_r0", _dp), ("iterations", C.c_int), ("applied", C.c_int), ("final_cost", C.c_double)]


class SnapshotTd(C.Structure):    # tcv_window_snapshot_td (include/tcv_estimator_td.h)
    _fields_ = [("estimate_td", C.c_int), ("n_proj", C.c_int), ("td_in", C.c_double), ("td_out", C.c_double), ("TR", C.c_double), ("ROW", C.c_double),
                ("proj_td_aux", _dp)]


KINDS = {0: "pose", 1: "sb", 2: "ex", 3: "td"}


def snapshot_window(tcv, S, T=None):
    """both snapshots -> the window dict the oracles take (the shape of tests/test_gpu_teacher.py's, plus `td` and the TD fields of
    synth.with_time_offset in `proj` when T says estimate_td), and the native results"""
    arr = lambda p, n, shape=None: np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape or (n,)) if n else np.zeros(shape or (0,))
    iarr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).astype(np.int64).copy() if n else np.zeros(0, np.int64)
    F, L, NI, NP, NL = S.n_frames, S.n_landmarks, S.n_imu, S.n_proj, S.n_line
    pre = (tcv.ImuPreintegration * max(1, NI)).from_address(S.imu) if NI else []
    col = lambda f, w: np.array([list(getattr(pre[k], f)) for k in range(NI)]).reshape((NI,) + w)
    imu = {"delta_p": col("delta_p", (3,)), "delta_q": col("delta_q", (4,)), "delta_v": col("delta_v", (3,)), "lin_ba": col("linearized_ba", (3,)),
           "lin_bg": col("linearized_bg", (3,)), "sum_dt": np.array([pre[k].sum_dt for k in range(NI)]), "jacobian": col("jacobian", (15, 15)),
           "covariance": col("covariance", (15, 15)), "frame_i": iarr(S.imu_frame_i, NI), "frame_j": iarr(S.imu_frame_j, NI)}
    pts = arr(S.proj_pts, 6 * NP, (NP, 6))
    proj = dict(frame_i=iarr(S.proj_frame_i, NP), frame_j=iarr(S.proj_frame_j, NP), landmark=iarr(S.proj_feature, NP), pts_i=pts[:, :3].copy(), pts_j=pts[:, 3:].copy(),
                sqrt_info=S.proj_sqrt_info, loss_a=1.0)
    ld = arr(S.line_data, 9 * NL, (NL, 9))
    line = dict(frame=iarr(S.line_frame, NL), pts_start=ld[:, :3].copy(), pts_end=ld[:, 3:6].copy(), abc=ld[:, 6:].copy(), K=np.array(list(S.line_K)).reshape(3, 3),
                Ric=np.array(list(S.line_Ric)).reshape(3, 3), Tic=np.array(list(S.line_Tic)), loss_a=1.0, exact_jacobian=bool(S.line_exact_jacobian))
    prior = None
    if S.prior_n > 0:
        nb, n = S.prior_nblk, S.prior_n
        sizes = [int(v) for v in iarr(S.prior_block_size, nb)]
        x0 = arr(S.prior_x0, sum(sizes))
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        prior = dict(m=S.prior_m, n=n, sizes=sizes, idx=[int(v) - S.prior_m for v in iarr(S.prior_block_idx, nb)], x0=[x0[offs[k]:offs[k + 1]].copy() for k in range(nb)],
                     J0=arr(S.prior_J0, n * n, (n, n)).T.copy(), r0=arr(S.prior_r0, n),          # (column-major on the wire)
                     blocks=[(KINDS[int(k)], int(i)) for k, i in zip(iarr(S.prior_block_kind, nb), iarr(S.prior_block_index, nb))])
    win = dict(pose=arr(S.pose_in, 7 * F, (F, 7)), speedbias=arr(S.speedbias_in, 9 * F, (F, 9)), ex_pose=arr(S.ex_pose_in, 7), lam=arr(S.feature_in, L),
               imu=imu, proj=proj, line=line, G=np.array(list(S.gravity)), prior=prior)
    res = dict(pose=arr(S.pose_out, 7 * F, (F, 7)), sb=arr(S.speedbias_out, 9 * F, (F, 9)), ex=arr(S.ex_pose_out, 7), lam=arr(S.feature_out, L),
               iterations=S.iterations, cost=S.final_cost, applied=S.applied, flag=S.marg_flag, td=None)
    if T is not None and T.estimate_td:
        assert T.n_proj == NP
        aux = arr(T.proj_td_aux, 8 * NP, (NP, 8))      # tcv_window_desc::proj_td_aux: velocity_i xy, velocity_j xy, td_i, td_j, row_i, row_j
        proj.update(vel_i=aux[:, 0:2].copy(), vel_j=aux[:, 2:4].copy(), td_i=aux[:, 4].copy(), td_j=aux[:, 5].copy(), row_i=aux[:, 6].copy(), row_j=aux[:, 7].copy(),
                    TR=float(T.TR), ROW=float(T.ROW))
        win["td"] = float(T.td_in)
        res["td"] = float(T.td_out)
    return win, res


def run_native(tcv, streams, tap=(), num_iterations=8, fixed_iterations=True, **kw):
    """the streams in one lock-step list through the native estimator.  Per stream: dict(p, q, v, log -- replay.NativeLockstep.results() --,
    td = the estimator's td after every window, wins = [(window dict, native results)] of the tapped streams)"""
    import replay
    ls = replay.NativeLockstep(streams, num_iterations=num_iterations, fixed_iterations=fixed_iterations, **kw)
    L = tcv.lib()
    L.tcv_estimator_set_window_tap.argtypes = [C.c_void_p, C.c_int]
    L.tcv_estimator_get_window_snapshot.argtypes = [C.c_void_p, C.POINTER(Snapshot)]
    have_td = getattr(L, "tcv_estimator_get_window_snapshot_td", None) is not None
    if have_td:
        L.tcv_estimator_get_window_snapshot_td.argtypes = [C.c_void_p, C.POINTER(SnapshotTd)]
    out = [dict(td=[], wins=[]) for _ in streams]
    try:
        for si in tap:
            tcv.check(L.tcv_estimator_set_window_tap(ls.ests[si], 1))
        for k in range(ls.n_frames):
            if not ls.step(k):
                continue
            for si in range(len(streams)):
                if have_td:
                    out[si]["td"].append(ls.time_offset(si))
                if si in tap:
                    S, T = Snapshot(), SnapshotTd()
                    tcv.check(L.tcv_estimator_get_window_snapshot(ls.ests[si], C.byref(S)))
                    if have_td:
                        tcv.check(L.tcv_estimator_get_window_snapshot_td(ls.ests[si], C.byref(T)))
                    out[si]["wins"].append(snapshot_window(tcv, S, T if have_td else None))
        for o, r in zip(out, ls.results()):
            o.update(r)
    finally:
        ls.close()
    return out


def published(o):
    """every published state and every per-window statistic of one stream of run_native, as arrays (for np.array_equal)"""
    keys = sorted(o["log"][0]) if o["log"] else []
    return [o["t"], o["p"], o["q"], o["v"], np.array(o["td"])] + [np.array([w[k] for w in o["log"]]) for k in keys]


# ---- the oracle's answer to a window, on worker processes ---------------------------------------------------------------------------
def solve_window(paths, win, num_iterations=8, fixed_iterations=True):
    """NO.Problem / NO.solve on the window, then the gauge fix of double2vector (estimator.cpp:1537-1581)"""
    for p in paths:
        if p not in sys.path:
            sys.path.append(p)
    import np_oracle as NO
    x, so = NO.solve(NO.Problem(win), num_iterations, fixed_iterations)
    Rs, Ps, Vs, po = NO.gauge_fix(NO.q2R(win["pose"][0, 3:]), win["pose"][0, :3], x["pose"], x["sb"])
    sb = x["sb"].copy(); sb[:, :3] = Vs
    return dict(iterations=len(so["iterations"]), cost=float(so["final_cost"]), pose=po, sb=sb, ex=x["ex"], lam=x["lam"],
                td=None if "td" not in x else float(x["td"][0]))


_pool = None


def solve_windows(wins, num_iterations=8, fixed_iterations=True):
    """solve_window for every window, on up to 14 worker processes (spawned: they import NumPy and the oracle, nothing of the product)"""
    global _pool
    paths = [p for p in sys.path if p]
    if _pool is None and not os.environ.get("TCV_TEST_NO_POOL"):
        try:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            keys = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")      # (one thread per worker: they inherit the environment when they start)
            saved = {k: os.environ.get(k) for k in keys}
            os.environ.update({k: "1" for k in keys})
            try:
                _pool = ProcessPoolExecutor(max_workers=max(1, min(14, cores - 1)), mp_context=mp.get_context("spawn"))
                futs = [_pool.submit(solve_window, paths, w, num_iterations, fixed_iterations) for w in wins]
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            return [f.result(timeout=600) for f in futs]
        except Exception as e:      # noqa: BLE001 -- no pool: compute in this process
            print("td_oracle: worker pool unavailable (%s), solving in-process" % e)
            _pool = None
    if _pool is not None:
        return [f.result(timeout=600) for f in [_pool.submit(solve_window, paths, w, num_iterations, fixed_iterations) for w in wins]]
    return [solve_window(paths, w, num_iterations, fixed_iterations) for w in wins]


def compare(wins, sols):
    """per-window gates of the issue: (windows whose iteration counts differ, worst relative figures)"""
    from util import rel
    worst = dict(cost=0.0, pose=0.0, sb=0.0, ex=0.0, lam=0.0, td=0.0)
    bad_it = []
    for k, ((win, res), o) in enumerate(zip(wins, sols)):
        if o["iterations"] != res["iterations"]:
            bad_it.append((k, res["iterations"], o["iterations"]))
            continue
        worst["cost"] = max(worst["cost"], abs(res["cost"] - o["cost"]) / abs(o["cost"]))
        worst["pose"] = max(worst["pose"], rel(res["pose"], o["pose"])); worst["sb"] = max(worst["sb"], rel(res["sb"], o["sb"]))
        worst["ex"] = max(worst["ex"], rel(res["ex"], o["ex"])); worst["lam"] = max(worst["lam"], rel(res["lam"], o["lam"]))
        if o["td"] is not None:
            worst["td"] = max(worst["td"], abs(res["td"] - o["td"]) / max(1e-3, abs(o["td"])))      # tests/test_gpu_td.py:44-45
    return bad_it, worst
