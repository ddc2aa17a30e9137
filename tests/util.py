"""Shared helpers for the tests: golden-vector loading and small comparison utilities."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)


def rel(a, b):
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    if a.size == 0 and b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def fro(a, b):
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- parity per parameter family: every block of small magnitude (biases, inverse depths, extrinsic translation, td) is measured against
# its own reference magnitude, not against the largest block of the vector it is stored in
_STATE_PARTS = {"pose": (("p", 0, 3), ("q", 3, 7)), "sb": (("v", 0, 3), ("ba", 3, 6), ("bg", 6, 9)), "ex": (("p", 0, 3), ("q", 3, 7)),
                "relo": (("p", 0, 3), ("q", 3, 7))}
_TANGENT_PARTS = {"pose": (("p", 0, 3), ("th", 3, 6)), "sb": (("v", 0, 3), ("ba", 3, 6), ("bg", 6, 9)), "ex": (("ex_p", 0, 3), ("ex_th", 3, 6)),
                  "td": (("td", 0, 1),), "relo": (("relo_p", 0, 3), ("relo_th", 3, 6)), "lam": (("lam", 0, 1),)}


def state_families(states):
    """name -> array: pose.p, pose.q, sb.v, sb.ba, sb.bg, ex.p, ex.q, lam, and td, relo.p, relo.q when the states hold them"""
    out = {}
    for key in ("pose", "sb", "ex", "relo"):
        if states.get(key) is None:
            continue
        a = np.asarray(states[key], dtype=float)
        for name, lo, hi in _STATE_PARTS[key]:
            out[key + "." + name] = a[..., lo:hi]
    if states.get("lam") is not None:
        out["lam"] = np.asarray(states["lam"], dtype=float)
    if states.get("td") is not None:
        out["td"] = np.atleast_1d(np.asarray(states["td"], dtype=float))
    return out


def _index_families(entries):
    """entries: (block name, tangent offset) -> name -> sorted index array"""
    fam = {}
    for nm, lo in entries:
        for name, a, b in _TANGENT_PARTS[nm]:
            fam.setdefault(name, []).extend(range(lo + a, lo + b))
    return {k: np.array(v, dtype=int) for k, v in fam.items()}


def tangent_families(problem):
    """name -> indices into a tangent vector of an np_oracle.Problem (gradient, first step): p, th, v, ba, bg pooled over the frames,
    ex_p, ex_th, td, relo_p, relo_th, lam.  The layout is the problem's own (blocks, loff); a constant block has no entries."""
    return _index_families([(nm, problem.loff[(nm, i)]) for (nm, i, g) in problem.blocks if problem.loff[(nm, i)] >= 0])


def prior_families(prior):
    """the same over the kept blocks of a prior (blocks, idx): indices into b', r0 and the rows and columns of A'"""
    return _index_families([(nm, int(lo)) for (nm, i), lo in zip(prior["blocks"], prior["idx"])])


def prior_diagonal_blocks(A, prior):
    """name -> the diagonal blocks of A' (n x n) that belong to one family, pooled over the kept blocks and flattened"""
    A = np.asarray(A, dtype=float)
    out = {}
    for (nm, i), lo in zip(prior["blocks"], prior["idx"]):
        for name, a, b in _TANGENT_PARTS[nm]:
            out.setdefault(name, []).append(A[lo + a:lo + b, lo + a:lo + b].ravel())
    return {k: np.concatenate(v) for k, v in out.items()}


def _by_family(a, b, fam, dist):
    if fam is None:
        assert sorted(a) == sorted(b), (sorted(a), sorted(b))
        pairs = [(k, a[k], b[k]) for k in b]
    else:
        a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
        assert a.shape == b.shape, (a.shape, b.shape)
        pairs = [(k, a[ix], b[ix]) for k, ix in fam.items()]
    out = {}
    for k, x, y in pairs:
        x = np.asarray(x, dtype=float); y = np.asarray(y, dtype=float)
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if y.size == 0:
            continue
        if not np.any(y):          # nothing to be relative to: exact zeros are expected
            out[k] = 0.0 if not np.any(x) else float("inf")
            continue
        out[k] = dist(x, y)
    return out


def rel_by_family(a, b, fam=None):
    """name -> max |a - b| / max |b| within each family, b the reference.  a, b: vectors with `fam` name -> indices (tangent_families,
    prior_families), or two dicts name -> array (state_families, prior_diagonal_blocks).  An empty family is left out; where the
    reference is exactly zero the other side has to be exactly zero (inf otherwise)."""
    return _by_family(a, b, fam, lambda x, y: float(np.abs(x - y).max() / np.abs(y).max()))


def fro_by_family(a, b, fam=None):
    """the same with |a - b|_2 / |b|_2"""
    return _by_family(a, b, fam, lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y)))


def fmt_families(d):
    return " ".join("%s %.1e" % (k, v) for k, v in d.items())


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def golden_windows():
    """(pre window, main window with the golden prior, npz) from tests/golden/window.npz."""
    from make_golden import unflatten_window
    z = load("window.npz")
    pre = unflatten_window(z, "pre_"); main = unflatten_window(z, "main_")
    kinds = {0: "pose", 1: "sb", 2: "ex"}
    sizes = [int(s) for s in z["marg_sizes"]]
    x0, o = [], 0
    for s in sizes:
        x0.append(z["marg_x0"][o:o + s].copy()); o += s
    main["prior"] = dict(m=int(z["marg_m"]), n=int(z["marg_n"]), sizes=sizes, idx=[int(i) for i in z["marg_idx"]], x0=x0,
                         J0=z["marg_J0"], r0=z["marg_r0"],
                         blocks=[(kinds[int(k)], int(i)) for k, i in zip(z["marg_block_kind"], z["marg_block_index"])])
    return pre, main, z


def imu_pre(z, k, prefix="i1_"):
    return dict(delta_p=z[prefix + "delta_p"][k], delta_q=z[prefix + "delta_q"][k], delta_v=z[prefix + "delta_v"][k],
                lin_ba=z[prefix + "lin_ba"][k], lin_bg=z[prefix + "lin_bg"][k], sum_dt=float(z[prefix + "sum_dt"][k]),
                jacobian=z[prefix + "jacobian"][k], covariance=z[prefix + "covariance"][k])


def sub_window(w, frames, keep_lines=True):
    """first `frames` frames of a window (ragged case: factors that touch later frames are dropped)."""
    out = dict(w)
    out["pose"] = w["pose"][:frames]; out["speedbias"] = w["speedbias"][:frames]
    im = w["imu"]; ki = [k for k in range(len(im["frame_i"])) if im["frame_j"][k] < frames]
    out["imu"] = {k: (np.asarray(v)[ki] if isinstance(v, np.ndarray) and v.shape[:1] == (len(im["frame_i"]),) else v) for k, v in im.items()}
    pr = w["proj"]; kp = [k for k in range(len(pr["frame_i"])) if pr["frame_j"][k] < frames]
    out["proj"] = {k: (np.asarray(v)[kp] if isinstance(v, np.ndarray) and v.shape[:1] == (len(pr["frame_i"]),) else v) for k, v in pr.items()}
    used = sorted(set(int(l) for l in out["proj"]["landmark"]))
    remap = {l: i for i, l in enumerate(used)}
    out["proj"]["landmark"] = np.array([remap[int(l)] for l in out["proj"]["landmark"]], int)
    out["lam"] = w["lam"][used]
    ln = w["line"]; kl = [k for k in range(len(ln["frame"])) if ln["frame"][k] < frames and keep_lines]
    out["line"] = {k: (np.asarray(v)[kl] if isinstance(v, np.ndarray) and v.shape[:1] == (len(ln["frame"]),) else v) for k, v in ln.items()}
    out["prior"] = None
    return out
