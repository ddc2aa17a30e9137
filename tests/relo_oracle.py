"""Helpers of the relocalisation tests: the NumPy restatement of the tail of Estimator::double2vector (estimator.cpp:1606-1624) on top of
np_oracle.gauge_fix / R2ypr / ypr2R / R2q, the figures the tests gate, a native lock-step replay with the window tap (the three snapshots of
every window) and the oracle's answer to such windows on worker processes (np_oracle takes seconds per window; the workers never touch the
device)."""
import atexit
import ctypes as C
import os
import sys

import numpy as np

import td_oracle as T

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
MATS = ("relo_r", "relo_t", "drift_correct_r", "drift_correct_t", "relo_relative_t")
YAWS = ("relo_relative_yaw", "drift_correct_yaw")


def normalize_angle(a):          # Utility::normalizeAngle, utility.h:135-143 (degrees)
    if a > 0:
        return a - 360.0 * np.floor((a + 180.0) / 360.0)
    return a + 360.0 * np.floor((-a + 180.0) / 360.0)


def relo_tail(R0, P0, pose0, pose_l, relo_pose, prev_relo_t, prev_relo_r):
    """estimator.cpp:1606-1620.  R0 / P0: Rs[0] / Ps[0] before the solve; pose0, pose_l, relo_pose: the solved, un-fixed para_Pose[0],
    para_Pose[relo_frame_local_index], relo_Pose.  Degrees, quaternion x y z w."""
    import np_oracle as NO
    Rs, Ps, _, _ = NO.gauge_fix(R0, P0, np.stack([pose0, pose_l, relo_pose]), np.zeros((3, 9)))      # rot_diff and the loop :1565-1571 for the three poses
    Rl, Pl, relo_r, relo_t = Rs[1], Ps[1], Rs[2], Ps[2]                                               # :1610-1613
    prev_relo_r = np.asarray(prev_relo_r, dtype=float).reshape(3, 3); prev_relo_t = np.asarray(prev_relo_t, dtype=float)
    yaw = NO.R2ypr(prev_relo_r)[0] - NO.R2ypr(relo_r)[0]                                              # :1615
    drift_r = NO.ypr2R([yaw, 0.0, 0.0])                                                               # :1616
    return dict(relo_r=relo_r, relo_t=relo_t, drift_correct_r=drift_r, drift_correct_t=prev_relo_t - drift_r @ relo_t,          # :1617
                relo_relative_t=relo_r.T @ (Pl - relo_t), relo_relative_q=NO.R2q(relo_r.T @ Rl),                                # :1618-1619
                relo_relative_yaw=float(normalize_angle(NO.R2ypr(Rl)[0] - NO.R2ypr(relo_r)[0])), drift_correct_yaw=float(yaw))  # :1620


def yaw_err(a, b):
    """|a - b| in degrees, modulo 360"""
    return float(abs((a - b + 180.0) % 360.0 - 180.0))


def unit(a, b):
    """max |a - b| relative to max(1, |b|)"""
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def record_errors(got, ref):
    """the figures the tests gate: relo_r, relo_t, relo_relative_t relative to their largest entry, drift_correct_r / _t relative to
    max(1, |.|), relo_relative_q as a rotation, the yaw scalars modulo 360"""
    import np_oracle as NO
    from util import rel
    e = {k: (unit if k.startswith("drift") else rel)(got[k], ref[k]) for k in MATS}      # (util.rel: the gauge gate's measure, tests/test_gpu_gauge.py)
    qa, qb = np.asarray(got["relo_relative_q"], dtype=float), np.asarray(ref["relo_relative_q"], dtype=float)
    e["relo_relative_q"] = float(np.abs(NO.q2R(qa / np.linalg.norm(qa)) - NO.q2R(qb / np.linalg.norm(qb))).max())
    for k in YAWS:
        e[k] = yaw_err(got[k], ref[k])
    return e


def displaced(R, p, yaw_deg=3.0, t=(0.5, -0.3, 0.1)):
    """D of the tests: a pose rotated about the vertical by yaw_deg and shifted by t -- where a drift-free pose graph would have the frame"""
    import np_oracle as NO
    Rz = NO.ypr2R([yaw_deg, 0.0, 0.0])
    return Rz @ np.asarray(R, dtype=float), Rz @ np.asarray(p, dtype=float) + np.asarray(t, dtype=float)


class SnapshotRelo(C.Structure):      # tcv_window_snapshot_relo (include/tcv_estimator_relo.h)
    _fields_ = [(k, C.c_int) for k in ("has_relo", "local_index", "n_relo", "frame_index", "frame_serial", "pad_")] + \
               [("relo_pose_in", C.c_double * 7), ("relo_pose_out", C.c_double * 7), ("relo_frame_i", _ip), ("relo_feature", _ip), ("relo_pts", _dp),
                ("prev_relo_t", C.c_double * 3), ("prev_relo_r", C.c_double * 9)]      # + result (tcv.ReloResult), appended by snapshot_type()


def snapshot_type(tcv):
    class S(C.Structure):
        _fields_ = SnapshotRelo._fields_ + [("result", tcv.ReloResult)]
    return S


def add_relo(win, res, R):
    """the relocalisation snapshot into the window dict (win["relo"] as np_oracle.Problem takes it, plus what the tail needs) and the results"""
    if not R.has_relo:
        return
    n = R.n_relo
    pts = np.ctypeslib.as_array(R.relo_pts, shape=(6 * n,)).copy().reshape(n, 6)
    win["relo"] = dict(pose=np.array(list(R.relo_pose_in)), frame_i=np.ctypeslib.as_array(R.relo_frame_i, shape=(n,)).astype(np.int64).copy(),
                       landmark=np.ctypeslib.as_array(R.relo_feature, shape=(n,)).astype(np.int64).copy(), pts_i=pts[:, :3].copy(), pts_j=pts[:, 3:].copy(),
                       local_index=int(R.local_index), prev_relo_t=np.array(list(R.prev_relo_t)), prev_relo_r=np.array(list(R.prev_relo_r)).reshape(3, 3),
                       frame_index=int(R.frame_index), frame_serial=int(R.frame_serial))
    res["relo"] = np.array(list(R.relo_pose_out))
    res["relo_result"] = R.result.as_dict()


def run_native(tcv, streams, tap=(), num_iterations=8, fixed_iterations=True, **kw):
    """td_oracle.run_native with the relocalisation part: the streams in one lock-step list through the native estimator.  Per stream:
    dict(p, q, v, log, relo = tcv_estimator_get_relocalization after every window, serials = the window's frame serials before every frame,
    wins = [(window dict, native results)] of the tapped streams, accepted = [(frame, accepted)] of its requests)"""
    import replay
    ls = replay.NativeLockstep(streams, num_iterations=num_iterations, fixed_iterations=fixed_iterations, **kw)
    L = tcv.lib()
    SR = snapshot_type(tcv)
    L.tcv_estimator_set_window_tap.argtypes = [C.c_void_p, C.c_int]
    L.tcv_estimator_get_window_snapshot.argtypes = [C.c_void_p, C.POINTER(T.Snapshot)]
    L.tcv_estimator_get_window_snapshot_relo.argtypes = [C.c_void_p, C.POINTER(SR)]
    out = [dict(relo=[], wins=[], serials=[]) for _ in streams]
    try:
        for si in tap:
            tcv.check(L.tcv_estimator_set_window_tap(ls.ests[si], 1))
        for k in range(ls.n_frames):
            for si in range(len(streams)):
                out[si]["serials"].append(ls.frame_serials(si))
            if not ls.step(k):
                continue
            for si in range(len(streams)):
                out[si]["relo"].append(ls.relocalization(si))
                if si in tap:
                    S, R = T.Snapshot(), SR()
                    tcv.check(L.tcv_estimator_get_window_snapshot(ls.ests[si], C.byref(S)))
                    tcv.check(L.tcv_estimator_get_window_snapshot_relo(ls.ests[si], C.byref(R)))
                    win, res = T.snapshot_window(tcv, S, None)
                    add_relo(win, res, R)
                    out[si]["wins"].append((win, res))
        for si, (o, r) in enumerate(zip(out, ls.results())):
            o.update(r)
            o["accepted"] = [(k, a) for k, s, a in ls.relo_accepted if s == si]
    finally:
        ls.close()
    return out


def published(o):
    """every published state and every per-window statistic of one stream of run_native, as arrays (for np.array_equal)"""
    keys = sorted(o["log"][0]) if o["log"] else []
    return [o["t"], o["p"], o["q"], o["v"]] + [np.array([w[k] for w in o["log"]]) for k in keys]


# ---- the oracle's answer to a window, on worker processes ---------------------------------------------------------------------------
def solve_window(paths, win, num_iterations=8, fixed_iterations=True):
    """NO.Problem / NO.solve on the window, the gauge fix of double2vector (estimator.cpp:1537-1581) and, for a relocalisation window, its tail"""
    for p in paths:
        if p not in sys.path:
            sys.path.append(p)
    import np_oracle as NO
    x, so = NO.solve(NO.Problem(win), num_iterations, fixed_iterations)
    pose_in = np.asarray(win["pose"], dtype=float)
    R0, P0 = NO.q2R(pose_in[0, 3:]), pose_in[0, :3]
    Rs, Ps, Vs, po = NO.gauge_fix(R0, P0, x["pose"], x["sb"])
    sb = x["sb"].copy(); sb[:, :3] = Vs
    out = dict(iterations=len(so["iterations"]), cost=float(so["final_cost"]), pose=po, sb=sb, ex=x["ex"], lam=x["lam"], td=None, raw_pose=x["pose"].copy())
    rl = win.get("relo")
    if rl is not None:
        out["relo"] = x["relo"].copy()
        if "local_index" in rl:
            out["relo_result"] = relo_tail(R0, P0, x["pose"][0], x["pose"][rl["local_index"]], x["relo"], rl["prev_relo_t"], rl["prev_relo_r"])
    return out


_pool = None


def _close_pool():
    if _pool is not None:
        _pool.shutdown(wait=False, cancel_futures=True)


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
                atexit.register(_close_pool)
                futs = [_pool.submit(solve_window, paths, w, num_iterations, fixed_iterations) for w in wins]
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            return [f.result(timeout=600) for f in futs]
        except Exception as e:      # noqa: BLE001 -- no pool: compute in this process
            print("relo_oracle: worker pool unavailable (%s), solving in-process" % e)
            _pool = None
    if _pool is not None:
        return [f.result(timeout=600) for f in [_pool.submit(solve_window, paths, w, num_iterations, fixed_iterations) for w in wins]]
    return [solve_window(paths, w, num_iterations, fixed_iterations) for w in wins]
