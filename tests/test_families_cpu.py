"""The per-family parity gates themselves, without a device (tests/util.py: state_families, tangent_families, prior_families,
rel_by_family, fro_by_family; tests/evaluate_cases.py: gradient_error_by_family).

A whole-vector `rel` / `fro` is relative to the largest block of the vector: the gyro-bias entries of a solved speed-bias array are 4e-5 of
its velocities, the inverse-depth entries of a window gradient 1e-6 of its rotation entries, the gyro-bias entries of a first step 3e-5 of
its norm.  Three things are pinned here: (1) the floor -- the two oracles (and the C oracle against the 50-digit first step) agree within
every family to a tenth of the gate the device is held to; (2) the power -- one family of the oracle's own output corrupted fails the
per-family check on every window, and passes the whole-vector check of before on the windows named below; (3) the layout -- the tangent
families partition the tangent vector of the four window kinds."""
import numpy as np
import pytest

import np_oracle as NO
import orc
import synth
from evaluate_cases import cases, gradient_error_by_family, oracle_evaluate
from util import (fmt_families, fro, fro_by_family, golden_windows, load, prior_diagonal_blocks, prior_families, rel, rel_by_family, state_families,
                  tangent_families)

GRAD_GATE, STATE_GATE, STEP_GATE = 1e-10, 1e-6, 1e-7          # what the device is held to (test_gpu_evaluate, test_gpu_solve, test_gpu_pins)


@pytest.fixture(scope="module")
def lib(built):
    return orc.lib()


@pytest.fixture(scope="module")
def evaluations(lib):
    """name -> (NumPy oracle's evaluation, C oracle's gradient) of every case the C oracle can evaluate; computed once, left unchanged"""
    out = {}
    for name, (w, kw) in cases().items():
        if any(w.get(k) is not None for k in ("td", "relo")) or w["line"].get("exact_jacobian"):
            continue          # the C oracle has no ProjectionTdFactor, relocalisation pose or exact line Jacobian
        exc = not kw.get("estimate_extrinsic", True)
        o = oracle_evaluate(w, ex_constant=exc)
        H, g, cost, n, nc = orc.Window(w, ex_constant=exc).linearize_dense()
        assert n == o["problem"].nlocal and nc == o["problem"].nc
        out[name] = (o, g)
    return out


def solve_windows():
    pre, main, z = golden_windows()
    return {"synth_200": synth.window_at(synth.make_windows(200, 1), 0), "synth_4242": synth.window_at(synth.make_windows(4242, 1), 0), "golden_main": main}


@pytest.fixture(scope="module")
def solutions(lib):
    """name -> (C oracle's states, NumPy oracle's states) after 8 fixed iterations; computed once, left unchanged"""
    out = {}
    for name, w in solve_windows().items():
        O = orc.Window(w); O.solve(8, True)
        x, _ = NO.solve(NO.Problem(w), 8, True)
        out[name] = (O.states(), x)
    return out


@pytest.fixture(scope="module")
def first_steps(lib):
    """name -> (C oracle's first step, the 50-digit first step, tangent families)"""
    pre, main, z = golden_windows()
    P = load("pins.npz")
    out = {}
    for w, p in ((pre, "pre_"), (main, "main_")):
        s = orc.Window(w).solve(1, True)
        out["golden_" + p[:-1]] = (np.array(s.first_delta[:s.n_local]), P["mp_" + p + "delta"], tangent_families(NO.Problem(w)))
    return out


# ---- (1) the floor of the references
def test_floor_gradient_of_the_two_oracles_per_entry(evaluations):
    worst = {}
    for name, (o, g) in evaluations.items():
        byf = gradient_error_by_family(g, o)
        print("%-24s gradient, C oracle against NumPy oracle, / |J|'|r|: %s" % (name, fmt_families(byf)))
        for fam, v in byf.items():
            worst[fam] = max(worst.get(fam, 0.0), v)
            assert v <= 0.1 * GRAD_GATE, (name, fam, v)          # measured worst 7.3e-13
    assert set(worst) == {"p", "th", "v", "ba", "bg", "ex_p", "ex_th", "lam"}


def test_floor_solved_states_of_the_two_oracles_per_family(solutions):
    for name, (sc, sn) in solutions.items():
        byf = rel_by_family(state_families(sn), state_families(sc))
        print("%-12s solved states, NumPy oracle against C oracle: %s" % (name, fmt_families(byf)))
        assert set(byf) == {"pose.p", "pose.q", "sb.v", "sb.ba", "sb.bg", "ex.p", "ex.q", "lam"}
        for fam, v in byf.items():
            assert v <= 0.1 * STATE_GATE, (name, fam, v)          # measured worst 1.1e-8 (sb.ba, sb.bg of synth_4242)


def test_floor_first_step_of_the_c_oracle_against_50_digits_per_family(first_steps):
    for name, (d, pin, fam) in first_steps.items():
        byf = fro_by_family(d, pin, fam)
        print("%-12s first step, C oracle against the 50-digit solution: %s" % (name, fmt_families(byf)))
        for f, v in byf.items():
            assert v <= 0.1 * STEP_GATE, (name, f, v)          # measured worst 7.3e-9 (ba of golden_main)


# ---- (2) the power of the gates: one family corrupted
# windows on which the whole-vector check of before (max(rel, fro) < 1e-6 on the gradient, rel < 1e-6 on the speed-bias array, fro < 1e-7 on the
# first step) accepts the corrupted output
OLD_GATE_PASSES = {
    "gradient": ("golden_main", "synth_lines_no_prior", "constant_extrinsic", "ragged_3", "ragged_6", "ragged_9"),
    "speed-bias": ("synth_200", "synth_4242", "golden_main"),
    "first step": ("golden_pre",),          # (golden_main: 1.4e-7, the whole-step check of before sees it)
}


def test_power_gradient_without_its_inverse_depth_part(evaluations):
    """a kernel that never accumulated the inverse-depth gradient"""
    passed_before = []
    for name, (o, _) in evaluations.items():
        lam = tangent_families(o["problem"]).get("lam", np.zeros(0, int))
        if len(lam) == 0:
            continue
        g = o["gradient"].copy(); g[lam] = 0.0
        old = max(rel(g, o["gradient"]), fro(g, o["gradient"]))
        byf = gradient_error_by_family(g, o)
        print("%-24s lam part zeroed: whole-vector %.2e, per entry in lam %.2e" % (name, old, byf["lam"]))
        assert byf["lam"] > GRAD_GATE and all(v == 0.0 for f, v in byf.items() if f != "lam"), (name, byf)
        if old < 1e-6:
            passed_before.append(name)
    assert set(OLD_GATE_PASSES["gradient"]) <= set(passed_before), passed_before


def test_power_gyro_bias_of_the_solved_states_off_by_a_hundredth(solutions):
    passed_before = []
    for name, (sc, _) in solutions.items():
        sb = sc["sb"].copy(); sb[:, 6:9] *= 1.01
        old = rel(sb, sc["sb"])
        byf = rel_by_family(state_families(dict(sc, sb=sb)), state_families(sc))
        print("%-12s bg x 1.01: whole speed-bias array %.2e, per family %s" % (name, old, fmt_families(byf)))
        assert byf["sb.bg"] > STATE_GATE and all(v == 0.0 for f, v in byf.items() if f != "sb.bg"), (name, byf)
        if old < 1e-6:
            passed_before.append(name)
    assert set(OLD_GATE_PASSES["speed-bias"]) <= set(passed_before), passed_before


def test_power_gyro_bias_of_the_first_step_off_by_a_thousandth(first_steps):
    passed_before = []
    for name, (d, pin, fam) in first_steps.items():
        c = d.copy(); c[fam["bg"]] *= 1.001
        old = fro(c, pin)
        byf = fro_by_family(c, pin, fam)
        print("%-12s bg x 1.001: whole step %.2e, bg family %.2e" % (name, old, byf["bg"]))
        assert byf["bg"] > STEP_GATE, (name, byf)
        if old < 1e-7:
            passed_before.append(name)
    assert set(OLD_GATE_PASSES["first step"]) <= set(passed_before), passed_before


# ---- (3) the layout
def test_tangent_families_partition_the_tangent_vector():
    cs = cases()
    expect = {"golden_main": (171, set()), "constant_extrinsic": (165, {"ex_p", "ex_th"}), "estimate_td": (172, set()), "relocalisation": (177, set())}
    for name, (nc, absent) in expect.items():
        w, kw = cs[name]
        P = NO.Problem(w, ex_constant=not kw.get("estimate_extrinsic", True))
        fam = tangent_families(P)
        ix = np.concatenate(list(fam.values()))
        assert sorted(ix) == list(range(P.nlocal)), name          # every index once
        assert P.nc == nc and sorted(fam["lam"]) == list(range(P.nc, P.nlocal)), name
        F = w["pose"].shape[0]
        assert all(len(fam[k]) == 3 * F for k in ("p", "th", "v", "ba", "bg")) and not absent & set(fam), name
        assert ("td" in fam) == (name == "estimate_td") and ("relo_p" in fam and "relo_th" in fam) == (name == "relocalisation"), name
        # ... and they are the problem's own blocks: a step along one family moves that family of the states and nothing else
        x = P.x0()
        for k, idx in fam.items():
            d = np.zeros(P.nlocal); d[idx] = 1e-3
            moved = {f for f, v in rel_by_family(state_families(P.plus(x, d)), state_families(x)).items() if v > 1e-9}          # (plus re-normalises every quaternion: 1e-16)
            want = {"p": "pose.p", "th": "pose.q", "v": "sb.v", "ba": "sb.ba", "bg": "sb.bg", "ex_p": "ex.p", "ex_th": "ex.q", "td": "td", "relo_p": "relo.p",
                    "relo_th": "relo.q", "lam": "lam"}[k]
            assert moved == {want}, (name, k, moved)


def test_prior_families_cover_the_kept_blocks_of_a_prior():
    pre, main, z = golden_windows()
    p = main["prior"]
    fam = prior_families(p)
    assert sorted(np.concatenate(list(fam.values()))) == list(range(p["n"]))
    assert set(fam) == {"p", "th", "v", "ba", "bg", "ex_p", "ex_th"} and len(fam["ba"]) == 3 and len(fam["p"]) == 30
    A = np.arange(p["n"] * p["n"], dtype=float).reshape(p["n"], p["n"])
    blocks = prior_diagonal_blocks(A, p)
    assert set(blocks) == set(fam) and all(len(blocks[k]) == 3 * len(fam[k]) for k in fam)
    assert np.array_equal(blocks["ba"], A[np.ix_(fam["ba"], fam["ba"])].ravel())


def test_zero_reference_and_empty_families():
    fam = {"a": np.array([0, 1]), "b": np.array([2]), "none": np.zeros(0, int)}
    ref = np.array([1.0, -2.0, 0.0])
    assert rel_by_family(ref, ref, fam) == {"a": 0.0, "b": 0.0} == fro_by_family(ref, ref, fam)
    assert rel_by_family(np.array([1.0, -2.0, 1e-300]), ref, fam)["b"] == float("inf")          # an exactly zero reference: exactly zero
    assert rel_by_family(np.array([1.0, -2.5, 0.0]), ref, fam) == {"a": 0.25, "b": 0.0}
    assert fro_by_family(np.array([1.0, -2.0, 0.0]) * 2, ref, fam)["a"] == 1.0
