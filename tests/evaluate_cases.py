"""Test helper for Problem::Evaluate (tests/test_gpu_evaluate.py, tests/evaluate_oracle_figures.py): the windows the parity gates run on and
the NumPy oracle's evaluation in the product's order -- the prior's rows, IMU, point (relocalisation factors behind the window's own:
they are added later), line."""
import numpy as np

import np_oracle as NO
import synth
from relo_util import add_relocalisation
from util import golden_windows, sub_window


def no_loss(w):
    """the window without its loss functions (apply_loss_function = 0 is checked against the oracle on this copy)"""
    return dict(w, proj=dict(w["proj"], loss_a=None), line=dict(w["line"], loss_a=None))


def no_points(w):
    pr = w["proj"]
    n = len(pr["frame_i"])
    return dict(w, proj={k: (np.asarray(v)[:0] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in pr.items()}, lam=np.zeros(0))


def cases():
    """name -> (window dict, keyword arguments of tcv.Window / ex_constant of the oracle)"""
    pre, main, z = golden_windows()
    out = {"golden_pre": (pre, {}), "golden_main": (main, {})}
    b = synth.make_windows(100, 2, with_lines=False)
    out["synth_points_only"] = (synth.window_at(b, 0), {})
    b = synth.make_windows(200, 2)
    out["synth_lines_prior"] = (synth.window_at(b, 0), {})
    out["synth_lines_no_prior"] = (dict(synth.window_at(b, 1), prior=None), {})
    out["constant_extrinsic"] = (synth.window_at(synth.make_windows(300, 1), 0), dict(estimate_extrinsic=False))
    for frames in (3, 6, 9):
        out["ragged_%d" % frames] = (sub_window(synth.window_at(synth.make_windows(400, 1), 0), frames), {})
    out["no_points"] = (no_points(synth.window_at(synth.make_windows(500, 1), 0)), {})
    out["estimate_td"] = (synth.with_time_offset(synth.window_at(synth.make_windows(22, 1), 0), 22, TR=0.02), {})
    out["relocalisation"] = (add_relocalisation(main, f=4, seed=1), {})
    out["line_exact"] = (dict(synth.window_at(synth.make_windows(77, 1), 0), line=dict(synth.window_at(synth.make_windows(77, 1), 0)["line"], exact_jacobian=True)), {})
    return out


def oracle_state(P, W, relo=None):
    """the oracle's state dict at the CURRENT values of a tcv.Window's arrays"""
    x = dict(pose=W.pose.copy(), sb=W.sb.copy(), ex=W.ex.copy(), lam=W.lam.copy())
    if P.has_td:
        x["td"] = W.td.copy()
    if P.has_relo:
        x["relo"] = np.asarray(relo, dtype=float).copy()
    return x


def oracle_evaluate(w, x=None, ex_constant=False):
    """dict(cost, family_cost (4), residuals, block_costs, gradient) of np_oracle.Problem(w) at x (default: the window's own states), in the
    product's order; scale = |J|'|r| (the magnitude each gradient entry is summed from); row_family / block_family: the factor family
    (index into FACTOR_FAMILIES) of every residual row / residual block"""
    P = NO.Problem(w, ex_constant=ex_constant)
    x = P.x0() if x is None else x
    J, r, cost = P.linearize(x)
    g = J.T @ r
    scale = np.abs(J).T @ np.abs(r)
    fam_of = {"prior": 0, "imu": 1, "proj": 2, "proj_td": 2, "proj_relo": 2, "line": 3}
    rank = {"prior": 0, "imu": 1, "proj": 2, "proj_td": 2, "proj_relo": 3, "line": 4}
    rows, blocks, fam, o = [], [], np.zeros(4), 0
    for fac in P.factors():
        rf, _, c = P.eval_factor(fac, x, False)
        rows.append((rank[fac[0]], len(rows), np.arange(o, o + len(rf)))); blocks.append((rank[fac[0]], len(blocks), c))
        fam[fam_of[fac[0]]] += c
        o += len(rf)
    rows.sort(key=lambda t: (t[0], t[1])); blocks.sort(key=lambda t: (t[0], t[1]))
    idx = np.concatenate([t[2] for t in rows]) if rows else np.zeros(0, int)
    row_family = np.concatenate([np.full(len(t[2]), t[0]) for t in rows]) if rows else np.zeros(0, int)
    return dict(cost=cost, family_cost=fam, residuals=r[idx], block_costs=np.array([t[2] for t in blocks]), gradient=g, problem=P,
                scale=scale, row_family=row_family, block_family=np.array([t[0] for t in blocks], dtype=int))


FACTOR_FAMILIES = ("prior", "imu", "point", "relocalisation point", "line")          # (the `rank` of oracle_evaluate)


def factor_families(family):
    """name -> indices of the rows / blocks of each factor family, for util.rel_by_family"""
    return {name: np.nonzero(family == k)[0] for k, name in enumerate(FACTOR_FAMILIES) if np.any(family == k)}


def gradient_error_by_family(g, o):
    """name -> max_i |g - g_ref|_i / scale_i within each tangent family of the oracle's problem, scale = |J|'|r|: each product J_ki r_k is
    good to the factor evaluators' gate, so their sum is good to that gate times sum_k |J_ki| |r_k|.  Where the scale is exactly zero (a
    block no factor touches) the entry has to be exactly zero (inf otherwise)."""
    from util import tangent_families
    g = np.asarray(g, dtype=float)
    d, s = np.abs(g - o["gradient"]), o["scale"]
    out = {}
    for name, ix in tangent_families(o["problem"]).items():
        if len(ix) == 0:
            continue
        z = s[ix] == 0
        if np.any(g[ix][z] != 0):
            out[name] = float("inf")
            continue
        out[name] = float((d[ix][~z] / s[ix][~z]).max()) if np.any(~z) else 0.0
    return out


def oracle_gradient_movement(w, x, o, ex_constant=False):
    """name -> how far the NumPy oracle's OWN gradient moves, in the units of gradient_error_by_family, when the states x move by 1e-13
    relative (poses, speed-biases, inverse depths; three draws: the measure tests/dev/fuzz_solve.py oracle_sensitivity prices ill-posed
    windows with).  Near a minimum the residuals are small differences of large terms, so |J|'|r| shrinks while what a rounding of the
    states does to J'r does not."""
    out = {}
    for rep in range(3):
        rng = np.random.Generator(np.random.PCG64(977 + rep))
        x2 = dict(x)
        for key in ("pose", "sb", "lam"):
            a = np.asarray(x[key], dtype=float)
            x2[key] = a * (1 + 1e-13 * rng.standard_normal(a.shape))
        for name, v in gradient_error_by_family(oracle_evaluate(w, x2, ex_constant=ex_constant)["gradient"], o).items():
            out[name] = max(out.get(name, 0.0), v)
    return out


def directional_error(cost_at, g, plus, x, d, eps=1e-6):
    """|(cost(x + eps d) - cost(x - eps d)) / (2 eps) - g . d| / |g . d|"""
    dd = (cost_at(plus(x, eps * d)) - cost_at(plus(x, -eps * d))) / (2 * eps)
    gd = float(np.dot(g, d))
    return abs(dd - gd) / max(abs(gd), 1e-300)


def hip_window(tcv, w, **kw):
    """tcv.Window of a case; a relocalisation window gets its `relo_Pose` block and factors the way estimator.cpp:1854-1886 adds them
    (behind everything else).  Returns (window, relo pose array or None)."""
    W = tcv.Window(w, **kw)
    rl = w.get("relo")
    if rl is None:
        return W, None
    relo = tcv.f64(rl["pose"]).copy()
    L, pr, keep = tcv.lib(), w["proj"], []
    tcv.check(L.tcv_problem_add_parameter_block(W.h, tcv.dptr(relo), 7, tcv.TCV_PARAM_POSE))
    for k in range(len(rl["frame_i"])):
        pi, pj = tcv.f64(rl["pts_i"][k]).copy(), tcv.f64(rl["pts_j"][k]).copy()
        keep.append((pi, pj))
        tcv.check(L.tcv_problem_add_projection_factor(W.h, tcv.dptr(pi), tcv.dptr(pj), float(pr["sqrt_info"]), float(pr["loss_a"]), W.block_ptr("pose", int(rl["frame_i"][k])),
                                                      tcv.dptr(relo), tcv.dptr(W.ex), W.block_ptr("lam", int(rl["landmark"][k]))))
    W._relo_keep = (keep, relo)
    return W, relo
