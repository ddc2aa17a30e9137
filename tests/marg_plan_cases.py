"""The marginalisation problems whose packed plans tests/golden/marg_plans.npz pins (tests/test_marg_pack_cpu.py compares, tests/golden/
make_golden_marg_plans.py records): every case is packed by tcv_problem_marg_plan, without a device, stand-alone and next to its solve
problem.  A record holds the ints in full ([MargHdr | int pool]), the length of the double pool and a SHA-256 per double section
(d_x, d_imu, d_proj, d_prior, d_misc), or the return code and the error text of a case that is refused."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np

import synth
from util import golden_windows, sub_window

SECTIONS = ("d_x", "d_imu", "d_proj", "d_prior", "d_misc")
SWITCHES = ("TCV_MARG_PROJ_SERIAL", "TCV_MARG_BLOCK_SERIAL", "TCV_MARG_OWN_IMU", "TCV_MARG_OWN_PRIOR")
# the smallest synthetic front end whose MARGIN_OLD leaves the one-piece mode: landmark k is anchored in frame k % 7 (synth.track_table),
# so 344 landmarks anchor 50 in frame 0 and the dropped set has 6 + 9 + 50 = 65 > 64 dims (343: 49 landmarks, 64 dims, one piece);
# 50 eliminated landmarks are four chunks of at most 16
BLOCK_LANDMARKS = 344


def _rows(d, n, keep):
    return {k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _big(seed):
    return synth.window_at(synth.make_windows(seed, 1, n_landmarks=BLOCK_LANDMARKS, frame_shift=-1), 0)


def _old(tcv, w, ex=True, share_prior=True):
    """(solve window, MARGIN_OLD problem on the same state arrays -- and the same prior object --, its drop list)"""
    W = tcv.Window(w, estimate_extrinsic=ex)
    mw = tcv.margin_old_window(w)
    M = tcv.Window(mw, estimate_extrinsic=ex, share=W, prior=W.prior if share_prior else None)
    return W, M, tcv.margin_old_drops(W, mw)


def _second_new(tcv, w):
    W = tcv.Window(w)
    M = tcv.Window(tcv.margin_second_new_window(w), share=W, prior=W.prior)
    return W, M, tcv.margin_second_new_drops(W)


def _not_disjoint(tcv, w):
    """MARGIN_OLD's factors plus three anchored in frame 1: pose 1 is the second pose of the former and the first of the latter"""
    pr = w["proj"]
    fi = np.asarray(pr["frame_i"])
    keep = np.sort(np.concatenate([np.nonzero(fi == 0)[0], np.nonzero(fi == 1)[0][:3]]))
    W = tcv.Window(w)
    mw = tcv.margin_old_window(w)
    mw["proj"] = _rows(pr, len(fi), keep)
    M = tcv.Window(mw, share=W)
    return W, M, tcv.margin_old_drops(W, tcv.margin_old_window(w))


def _keeps_nothing(tcv, w):
    """the IMU factor (0, 1) alone, all four of its blocks dropped"""
    W = tcv.Window(w)
    mw = tcv.margin_old_window(w)
    mw["proj"] = _rows(mw["proj"], len(mw["proj"]["frame_i"]), np.zeros(0, int))
    M = tcv.Window(mw, share=W)
    return W, M, [W.block_ptr("pose", 0), W.block_ptr("sb", 0), W.block_ptr("pose", 1), W.block_ptr("sb", 1)]


def _bogus_drop(tcv, w):
    W, M, dr = _old(tcv, w)
    M._bogus = np.zeros(7)
    return W, M, dr + [tcv.dptr(M._bogus)]


def _with_lines(tcv, w):
    W = tcv.Window(w)
    M = tcv.Window(w, share=W, prior=W.prior)      # the whole window, line factors included, as the factor set
    return W, M, [W.block_ptr("pose", 0), W.block_ptr("sb", 0)]


def _untouched_drop(tcv, w):
    W, M, dr = _old(tcv, w)
    return W, M, [W.block_ptr("sb", W.sb.shape[0] - 1)]      # no factor of MARGIN_OLD touches the newest speed-bias block (no prior)


def _mixed_td(tcv, w):
    W, M, dr = _old(tcv, w)
    pr = M.win["proj"]
    M._pi0 = tcv.f64(pr["pts_i"][0]); M._pj0 = tcv.f64(pr["pts_j"][0])
    tcv.check(tcv.lib().tcv_problem_add_projection_factor(M.h, tcv.dptr(M._pi0), tcv.dptr(M._pj0), float(pr["sqrt_info"]), float(pr["loss_a"] or 0.0),
                                                          W.block_ptr("pose", int(pr["frame_i"][0])), W.block_ptr("pose", int(pr["frame_j"][0])),
                                                          W.block_ptr("ex", 0), W.block_ptr("lam", int(pr["landmark"][0]))))
    return W, M, dr


def cases(tcv):
    """name -> (builder: () -> (solve window, marginalisation problem, drops), environment switches)"""
    pre, main, z = golden_windows()
    td_main = synth.with_time_offset(main, 917)
    out = {
        "old_prior": (lambda: _old(tcv, main), {}),
        "old_pre": (lambda: _old(tcv, pre), {}),
        "old_own_prior_object": (lambda: _old(tcv, main, share_prior=False), {}),      # (an equal prior behind another handle: not shared)
        "second_new": (lambda: _second_new(tcv, main), {}),
        "const_extrinsic": (lambda: _old(tcv, main, ex=False), {}),
        "block": (lambda: _old(tcv, _big(902)), {}),
        "block_6_frames": (lambda: _old(tcv, sub_window(_big(902), 6)), {}),      # (n = 45: C finds no room in region P)
        "td_one_piece": (lambda: _old(tcv, td_main), {}),
        "td_block": (lambda: _old(tcv, synth.with_time_offset(_big(903), 903)), {}),
        "not_disjoint": (lambda: _not_disjoint(tcv, pre), {}),
        "keeps_nothing": (lambda: _keeps_nothing(tcv, pre), {}),
        "switch_proj_serial": (lambda: _old(tcv, main), {"TCV_MARG_PROJ_SERIAL": "1"}),
        "switch_block_serial": (lambda: _old(tcv, _big(902)), {"TCV_MARG_BLOCK_SERIAL": "1"}),
        "switch_own_imu": (lambda: _old(tcv, main), {"TCV_MARG_OWN_IMU": "1"}),
        "switch_own_prior": (lambda: _old(tcv, main), {"TCV_MARG_OWN_PRIOR": "1"}),
        "err_drop_not_in_problem": (lambda: _bogus_drop(tcv, pre), {}),
        "err_line_factors": (lambda: _with_lines(tcv, main), {}),
        "err_m0": (lambda: _untouched_drop(tcv, pre), {}),
        "err_mixed_td": (lambda: _mixed_td(tcv, td_main), {}),
    }
    return out


def record(tcv, build, env, with_solve):
    """one packed case as a dict of plain arrays (the npz entries)"""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        W, M, drops = build()
        try:
            H, ints, dbl = tcv.marg_plan(M, drops, W if with_solve else None)
        except tcv.TcvError as e:
            return dict(rc=np.array([e.status], np.int32), err=np.frombuffer(str(e).encode(), np.uint8))
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    sha = np.zeros((len(SECTIONS), 32), np.uint8)
    if H is not None:
        cut = [getattr(H, s) for s in SECTIONS] + [len(dbl)]
        assert cut == sorted(cut) and cut[0] == 0, cut
        for i in range(len(SECTIONS)):
            sha[i] = np.frombuffer(hashlib.sha256(dbl[cut[i]:cut[i + 1]].tobytes()).digest(), np.uint8)
    return dict(rc=np.array([0], np.int32), ints=ints, dlen=np.array([len(dbl)], np.int32), sha=sha)


def header(tcv, ints):
    return tcv.MargHdr.from_buffer_copy(np.ascontiguousarray(ints[:C.sizeof(tcv.MargHdr) // 4], np.int32).tobytes())
