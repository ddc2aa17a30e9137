"""Test helper for the termination paths of the solve loop (tests/test_termination_cpu.py, tests/test_gpu_termination.py): named windows on
which BOTH oracles end on each of the termination codes 0 .. 4 with a clear margin, and an oracle-free checker of a solver summary against
the trust-region loop's own arithmetic.

A case is (w_hip, w_orc, ex_constant, max_iterations, fixed): the window as the library gets it, as the oracles get it (they differ where
an IMU factor over 10 s is left out, tests/dev/fuzz_solve.py make_case), and the run.  The windows are structures of the fuzzer
(fuzz_solve.make_case, seeds below 100000: the recorded list) except `gradient`: no fuzz structure ends on the gradient tolerance (the
function tolerance 1e-6 x cost always comes first when the cost at the minimum is not tiny), so that one is a window whose only factor is a
well-conditioned prior with a small residual -- a quadratic in the tangent, solved to |g|_inf <= 1e-10 in a few Gauss-Newton steps while the
cost still falls by orders of magnitude.  `gradient_landmarks_only` is that window with eight landmarks at a state where the camera part of
the gradient is 1e-13 and one landmark's entry 4e-10 (landmark_gradient_window): the gradient test has to read the landmark part.  `function` (seed 59: 23 landmarks, 4 line factors; 12 accepted and 12 rejected steps through all
three dogleg cases) is the only structure of seeds 0 .. 79 below 200 tangent dimensions that ends on the function tolerance with the
margins below; the suite's other function-tolerance runs (the golden window, the fuzzer's convergence mode) carry no such condition.

What ends each case, with the margins the CPU test asserts (deciding quantity <= 0.5 x its threshold, every quantity of every earlier
record >= 2 x): tests/test_termination_cpu.py prints them."""
import os
import sys
import types

import numpy as np

import np_oracle as NO
import orc
import synth
from util import golden_windows

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev"))
import fuzz_solve as fz      # noqa: E402

FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, GRADIENT_TOLERANCE, MIN_RADIUS, MIN_RELATIVE_DECREASE = 1e-6, 1e-8, 1e-10, 1e-32, 1e-3
NO_CONVERGENCE, GRADIENT, PARAMETER, FUNCTION, RADIUS, FAILURE = range(6)
LONG_TRACE = ("long_trace_seed0", "long_trace_seed17")
# name -> (termination both oracles end on, number of records)
EXPECTED = {"gradient": (GRADIENT, 4), "gradient_at_entry": (GRADIENT, 1), "gradient_landmarks_only": (FUNCTION, 2), "parameter_small": (PARAMETER, 6), "parameter_small2": (PARAMETER, 7),
            "parameter_small3": (PARAMETER, 5), "parameter_main": (PARAMETER, 24), "function": (FUNCTION, 25), "long_trace_seed0": (NO_CONVERGENCE, 101),
            "long_trace_seed17": (NO_CONVERGENCE, 101), "radius": (RADIUS, 124)}
_SEEDS = {"parameter_small": 132, "parameter_small2": 156, "parameter_small3": 20, "parameter_main": 264, "function": 59, "long_trace_seed0": 0,
          "long_trace_seed17": 17, "radius": 150}
_CACHE = {}


def fuzz_case(seed):
    w_hip, w_orc, exc, note = fz.make_case(np.random.Generator(np.random.PCG64(seed)), seed)
    return w_hip, w_orc, exc, note


def _empty(d, n):
    return fz.take(d, np.zeros(n, bool), n)


def prior_only_window():
    """golden `main` without point, line and IMU factors and without landmarks; the prior's J0, r0 replaced by a well-conditioned
    J0 = 1e-2 Q diag(1 .. 3) Q' and r0 = 1e-4 N(0, 1)"""
    pre, main, z = golden_windows()
    w = dict(main)
    w["proj"] = _empty({k: np.asarray(v) if isinstance(v, (list, np.ndarray)) else v for k, v in main["proj"].items()}, len(main["proj"]["landmark"]))
    w["line"] = _empty(main["line"], len(main["line"]["frame"]))
    w["imu"] = _empty(main["imu"], len(main["imu"]["sum_dt"]))
    w["lam"] = np.zeros(0)
    p = dict(main["prior"])
    n = int(p["n"])
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    p["J0"] = 1e-2 * Q @ np.diag(np.linspace(1.0, 3.0, n)) @ Q.T
    p["r0"] = 1e-4 * rng.normal(size=n)
    w["prior"] = p
    return w


def landmark_gradient_window(n_landmarks=8, seed=2, sqrt_info=1e-2, target=4e-10):
    """A state at which ONLY the landmark part of the gradient is above the gradient tolerance.  The prior-only window with eight of golden
    `main`'s landmarks and their point factors (weighted like the prior: sqrt_info 1e-2), taken to the C oracle's solved states (every
    gradient entry below 1e-10) and moved by Newton corrections H d = target - g, four times, towards the gradient `target` on the first
    landmark and zero everywhere else: camera part ~1e-13, landmark part 4e-10.  The loop must NOT stop on the gradient test before the
    first iteration here; a gradient test that leaves the landmarks out does."""
    pre, main, z = golden_windows()
    rng = np.random.default_rng(seed)
    pr = {k: np.asarray(v) if isinstance(v, (list, np.ndarray)) else v for k, v in main["proj"].items()}
    lms = sorted(int(l) for l in rng.choice(len(main["lam"]), n_landmarks, replace=False))
    p2 = fz.take(pr, np.isin(pr["landmark"], lms), len(pr["landmark"]))
    remap = {l: i for i, l in enumerate(lms)}
    p2["landmark"] = np.array([remap[int(l)] for l in p2["landmark"]], int)
    p2["sqrt_info"] = sqrt_info
    w = dict(prior_only_window(), proj=p2, lam=np.asarray(main["lam"])[lms].copy())
    O = orc.Window(w); O.solve(50, False)
    w = at_states(w, O.states())
    P = NO.Problem(w)
    x = P.x0()
    for _ in range(4):
        J, r, _cost = P.linearize(x)
        t = -(J.T @ r)
        t[P.nc] += target
        x = P.plus(x, np.linalg.lstsq(J.T @ J, t, rcond=1e-12)[0])
    return at_states(w, x)


def gradient_parts(w, ex_constant=False):
    """(max |g| over the camera part, over the landmark part) of the unscaled gradient at the window's own states (np_oracle)"""
    P = NO.Problem(w, ex_constant=ex_constant)
    J, r, _cost = P.linearize(P.x0())
    g = np.abs(J.T @ r)
    return float(g[:P.nc].max()), float(g[P.nc:].max()) if len(g) > P.nc else 0.0


def at_states(w, st):
    out = dict(w, pose=st["pose"].copy(), speedbias=st["sb"].copy(), ex_pose=st["ex"].copy(), lam=st["lam"].copy())
    if "td" in w and st.get("td") is not None:
        out["td"] = float(np.atleast_1d(st["td"])[0])
    return out


def cases():
    """name -> (w_hip, w_orc, ex_constant, max_iterations, fixed)"""
    if _CACHE:
        return dict(_CACHE)
    out = {}
    g = prior_only_window()
    out["gradient"] = (g, g, False, 50, False)
    O = orc.Window(g); O.solve(50, False)
    ge = at_states(g, O.states())
    out["gradient_at_entry"] = (ge, ge, False, 50, False)
    gl = landmark_gradient_window()
    out["gradient_landmarks_only"] = (gl, gl, False, 50, False)
    for name, seed in _SEEDS.items():
        w_hip, w_orc, exc, _ = fuzz_case(seed)
        out[name] = (w_hip, w_orc, exc, 130, True) if name == "radius" else (w_hip, w_orc, exc, 100, False)
    _CACHE.update(out)
    return dict(out)


TD_SEED, TD_TR = 41, 0.02


def td_window():
    """one ESTIMATE_TD window (every point factor a ProjectionTdFactor, tests/test_gpu_td.py): run (100, to convergence) against
    np_oracle.solve -- the C oracle has no ProjectionTdFactor"""
    return synth.with_time_offset(synth.window_at(synth.make_windows(TD_SEED, 1), 0), TD_SEED, TR=TD_TR)


perturbed = fz.perturbed      # the window with its states moved by 1e-13 relative: draw `rep` of fuzz_solve.oracle_sensitivity


def trace_of(s):
    """(num_iterations, termination, dogleg cases, accepts) of a C-oracle or device summary over the stored records"""
    n = min(s.num_iterations, len(s.step_ok))
    return (s.num_iterations, s.termination, tuple(s.dogleg_case[i] for i in range(1, n)), tuple(s.step_ok[i] for i in range(1, n)))


def np_trace_of(so):
    its = so["iterations"]
    return (len(its), so["termination_code"], tuple(int(r.get("case", 0)) for r in its[1:]), tuple(int(bool(r.get("step_ok", False))) for r in its[1:]))


def np_summary(so):
    """np_oracle's summary in the shape of the C summaries (attribute arrays over the records): the record of a convergence stop gets the
    rho the C oracle and the device record there (formed before the tests), step_ok 0"""
    its = so["iterations"]
    n = len(its)
    s = types.SimpleNamespace(num_iterations=n, termination=so["termination_code"], initial_cost=so["initial_cost"], final_cost=so["final_cost"])
    for f in ("cost", "cost_candidate", "model_cost_change", "radius", "mu", "rho", "step_norm"):
        setattr(s, f, [0.0] * n)
    s.step_ok, s.dogleg_case = [0] * n, [0] * n
    s.cost[0], s.step_ok[0] = its[0]["cost"], 1
    for i in range(1, n):
        r = its[i]
        s.cost[i] = r["cost"]; s.step_ok[i] = int(bool(r.get("step_ok", False))); s.dogleg_case[i] = int(r.get("case", -1)); s.mu[i] = r["mu"]
        if "model_cost_change" in r:
            s.cost_candidate[i], s.model_cost_change[i], s.radius[i], s.step_norm[i] = r["cost_candidate"], r["model_cost_change"], r["radius"], r["step_norm_dogleg"]
            s.rho[i] = r["rho"] if "rho" in r else (s.cost[i - 1] - r["cost_candidate"]) / r["model_cost_change"]
    return s


def decision_margins(so):
    """per record of an np_oracle summary, the three tested quantities over their thresholds: (parameter, function, gradient).  Record 0
    has the gradient ratio only (the test before the first iteration); the function ratio is |cost - cost_candidate| / (1e-6 cost) at
    the cost the iteration started from; the gradient ratio is the one the test after this record sees (unchanged by a rejected step)."""
    its = so["iterations"]
    out = [(float("inf"), float("inf"), its[0]["gradient_max_norm"] / GRADIENT_TOLERANCE)]
    for i in range(1, len(its)):
        r = its[i]
        if "cost_candidate" not in r:      # an invalid step: nothing is tested
            out.append((float("inf"), float("inf"), r["gradient_max_norm"] / GRADIENT_TOLERANCE))
            continue
        c0 = its[i - 1]["cost"]
        out.append((r["dx_norm"] / (PARAMETER_TOLERANCE * (r["x_norm"] + PARAMETER_TOLERANCE)),
                    abs(c0 - r["cost_candidate"]) / (FUNCTION_TOLERANCE * c0) if c0 > 0 else float("inf"),
                    r["gradient_max_norm"] / GRADIENT_TOLERANCE))
    return out


def check_margins(so, lo=2.0, hi=0.5):
    """the decisions of a convergence run are clear: at the deciding record the deciding quantity is <= hi x its threshold, at every earlier
    record all three tested quantities are >= lo x theirs (at the deciding record: those tested BEFORE the deciding one -- the loop tests
    parameter, function, gradient in that order).  Returns (deciding ratio, smallest other ratio) for the report."""
    m = decision_margins(so)
    t = so["termination_code"]
    assert t in (GRADIENT, PARAMETER, FUNCTION), t
    last = len(m) - 1
    others = [v for rec in m[:last] for v in rec]
    if t == GRADIENT:
        deciding = m[last][2]; others += [m[last][0], m[last][1]] if last > 0 else []
    elif t == PARAMETER:
        deciding = m[last][0]
    else:
        deciding = m[last][1]; others += [m[last][0]]
    least = min(others) if others else float("inf")
    assert deciding <= hi, ("deciding quantity / threshold", deciding)
    assert least >= lo, ("an earlier quantity / threshold", least)
    return deciding, least


def check_trace_rules(s, n_records):
    """A solver summary (device, C oracle, np_summary) against the loop's own arithmetic over its first n_records records; no oracle.
    The record of a convergence stop (termination 2 or 3: the last one) holds a candidate that was neither accepted nor rejected:
    step_ok is 0 there whatever rho says, and the cost is the one before."""
    n = int(n_records)
    assert 1 <= n <= s.num_iterations
    assert s.step_ok[0] == 1 and s.dogleg_case[0] == 0 and s.cost[0] == s.initial_cost
    if n > 1:
        assert s.radius[1] == 1e4
    for i in range(1, n):
        stop = s.termination in (PARAMETER, FUNCTION) and i == s.num_iterations - 1
        rho, rad, sn, case = s.rho[i], s.radius[i], s.step_norm[i], s.dogleg_case[i]
        assert s.mu[i] == 1e-8, (i, s.mu[i])
        assert s.model_cost_change[i] > 0, (i, s.model_cost_change[i])
        want = (s.cost[i - 1] - s.cost_candidate[i]) / s.model_cost_change[i]
        assert abs(rho - want) <= 1e-12 * abs(want), (i, rho, want)
        ok = int(s.step_ok[i])
        assert ok == (0 if stop else int(rho > MIN_RELATIVE_DECREASE)), (i, ok, rho)
        assert s.cost[i] == (s.cost_candidate[i] if ok else s.cost[i - 1]), (i, s.cost[i], s.cost_candidate[i], s.cost[i - 1])
        assert case in (1, 2, 3), (i, case)
        if case == 1:
            assert sn <= rad, (i, sn, rad)
        elif case == 2:
            assert sn == rad, (i, sn, rad)
        else:
            assert abs(sn - rad) <= 1e-9 * rad, (i, sn, rad)
        if i + 1 < n:
            if ok:
                nxt = rad * 0.5 if rho < 0.25 else rad
                if rho > 0.75:
                    nxt = max(nxt, 3.0 * sn)
            else:
                nxt = rad * 0.5
            assert s.radius[i + 1] == nxt, (i, s.radius[i + 1], nxt, rho, sn)
    if n == s.num_iterations:
        assert s.final_cost == s.cost[n - 1]
