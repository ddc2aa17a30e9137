"""Test helper for the batched marginal covariance: the windows and request lists the CPU and GPU tests share, and the references
(tests/covariance_oracle.py), each computed once per process.

The shapes are the smallest that reach every seam of the kernel (nc = camera-side tangent dimensions): 4 frames (66), 6 frames (96 =
six 16-wide tiles exactly), 6 frames + td (97), the full window (171), + td (172), constant extrinsic (165), relocalisation (177), the
golden window with its prior (prior_k0 > 0), and 200 landmarks.

The short windows are `util.sub_window`s with the IMU factors' bias random walk loosened 10x (covariance x 100).  As they come, a 4- or
6-frame window observes the biases so weakly against a random-walk information of 2e15 that its smallest relative Cholesky pivot is
3e-13 .. 2e-11 -- nearer to the rank gate than the 30x the gate's margin allows for a test input -- and a float64 inverse is off by
5e-3.  With the looser walk their pivots (5e-11, 1e-9) sit in the range of the full windows'.  What the short windows are for -- the
small sizes, the tile boundary -- does not depend on how hard the biases are tied."""
import functools

import numpy as np

import synth
from util import sub_window

import covariance_oracle as CO
import evaluate_cases as EC


def loose_bias_walk(w, scale=100.0):
    im = dict(w["imu"])
    cov = np.array(im["covariance"], dtype=float)
    cov[:, 9:15, 9:15] *= scale
    im["covariance"] = cov
    return dict(w, imu=im)


def no_gauge(seed):
    """a window with neither prior nor lines: nothing fixes the gauge, S is rank deficient (Covariance::Compute fails in Ceres)"""
    return dict(synth.window_at(synth.make_windows(seed, 1, with_lines=False), 0), prior=None)


NO_GAUGE_SEEDS = (9400, 9401, 9402)


@functools.lru_cache(maxsize=None)
def windows():
    """name -> (window dict, keyword arguments of tcv.Window)"""
    cs = EC.cases()
    base = synth.window_at(synth.make_windows(9400, 1), 0)
    six = loose_bias_walk(sub_window(base, 6))
    return {
        "frames4": (loose_bias_walk(sub_window(base, 4)), {}),
        "frames6": (six, {}),
        "frames6_td": (synth.with_time_offset(six, 22, TR=0.02), {}),
        "full": (base, {}),
        "full_td": cs["estimate_td"],
        "constant_extrinsic": cs["constant_extrinsic"],
        "relocalisation": cs["relocalisation"],
        "golden_prior": cs["golden_main"],
        "landmarks200": (synth.window_at(synth.make_windows(600, 1, n_landmarks=200), 0), {}),
    }


def requests(name):
    """the request list of a case: newest pose, newest pose x newest speed-bias (and its transpose), oldest pose, newest speed-bias,
    extrinsic, then td / the relocalisation pose where the window has one, then every pose"""
    w, kw = windows()[name]
    F = w["pose"].shape[0]
    rq = [(("pose", -1), ("pose", -1)), (("pose", -1), ("sb", -1)), (("sb", -1), ("pose", -1)), (("pose", 0), ("pose", 0)), (("sb", -1), ("sb", -1)),
          (("ex", 0), ("ex", 0)), (("ex", 0), ("pose", -1))]
    if w.get("td") is not None:
        rq += [(("td", 0), ("td", 0)), (("td", 0), ("pose", -1))]
    if w.get("relo") is not None:
        rq += [(("relo", 0), ("relo", 0)), (("relo", 0), ("pose", 4))]
    rq += [(("pose", i), ("pose", i)) for i in range(F)]
    return rq


_REF = {}


def reference(name, x=None, loss=True, key=None):
    """CO.Reference of a case at x (default: the window's own states), with or without the loss; cached under (name, loss, key)"""
    k = (name, loss, key)
    if k not in _REF:
        w, kw = windows()[name]
        _REF[k] = CO.Reference(w if loss else EC.no_loss(w), x, ex_constant=not kw.get("estimate_extrinsic", True))
    return _REF[k]


def device_order(P):
    """the kernel's elimination order over the oracle's camera-side tangent indices: the pose-kind blocks in block order, td, the speed-biases"""
    cam = [(nm, i, g) for (nm, i, g) in P.blocks if nm != "lam" and P.loff[(nm, i)] >= 0]
    ix = []
    for pick in (lambda nm: nm in ("pose", "ex", "relo"), lambda nm: nm == "td", lambda nm: nm == "sb"):
        for nm, i, g in cam:
            if pick(nm):
                lo = P.loff[(nm, i)]
                ix.extend(range(lo, lo + (6 if g == 7 else g)))
    return np.array(ix, dtype=int)
