"""Problem::Evaluate on the device (tcv_batch_evaluate / tcv_problem_evaluate, tc-viml_amd/csrc/tcv_eval.hip) against the two oracles as
they stand -- np_oracle.Problem.linearize (J, r, cost: gradient J'r) and orc.Window.linearize_dense (g, cost) --, the exact checks
(defined cost sum, run-to-run and batch-size independence bit for bit, no effect on what follows), consistency with the solver's
summary, the one-problem entry point, the C++ veneer and the leak check.  Gate: the project's TOL = 1e-6 (rel / fro of tests/util.py), on the
whole vectors and, for residuals and block costs, within each factor family; every gradient entry within GRAD_TOL = 1e-10 of (|J|'|r|)_i, the
sum it is formed from (a landmark entry is 1e-6 of the largest gradient entry: the whole-vector gate does not see it; tests/test_families_cpu.py).
At solved states the residuals are small differences of large terms and a family beyond GRAD_TOL is held to 30 x the oracle's own movement
under 1e-13 state noise (profiles/family_parity.txt: the gyro-bias entries, 2.7e-10).

Measured on an MI355X (profiles/evaluate_parity.txt; test_zz_report prints the worst figure per quantity): against the NumPy oracle cost
9.6e-16, residuals 1.8e-15, block costs 1.4e-15, gradient 1.2e-15; against the C oracle gradient 1.3e-15; the two oracles against each other
cost 7.6e-16, gradient 1.4e-15.  Directional derivative: oracle alone 8.6e-7 / 3.2e-9 (points only / exact line Jacobian), device 7.9e-7 / 2.8e-9."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import np_oracle as NO
import orc
import synth
from evaluate_cases import (cases, directional_error, factor_families, gradient_error_by_family, hip_window, no_loss, oracle_evaluate, oracle_gradient_movement,
                            oracle_state)
from util import fro, golden_windows, rel, rel_by_family, sub_window

pytestmark = pytest.mark.gpu
TOL = 1e-6
GRAD_TOL = 1e-10          # per gradient entry, in units of (|J|'|r|)_i: the gate of the factor evaluators (tests/test_gpu_factors.py TOL)
WORST = {}


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    return v


def both(a, b):
    return max(rel(a, b), fro(a, b))


def evaluate_one(gpu, W, **kw):
    b = gpu.Batch([W])
    b.evaluate(residuals=True, gradient=True, block_costs=True, **kw)
    return b, b.evaluation(0)


def check_vs_oracle(ev, o, tag, movement=None):
    """movement: None, or a function returning name -> the oracle's own movement of the gradient in that family under 1e-13 state noise
    (evaluate_cases.oracle_gradient_movement); a family beyond GRAD_TOL is then held to 30 x that movement, the allowance of
    tests/dev/fuzz_solve.py for reference-measured floors, and listed by test_zz_report"""
    assert note(tag + " cost", rel(ev["cost"], o["cost"])) < TOL
    assert note(tag + " family cost", rel(ev["family_cost"], o["family_cost"])) < TOL
    assert len(ev["residuals"]) == len(o["residuals"]) and note(tag + " residuals", both(ev["residuals"], o["residuals"])) < TOL
    assert len(ev["block_costs"]) == len(o["block_costs"]) and note(tag + " block costs", both(ev["block_costs"], o["block_costs"])) < TOL
    assert len(ev["gradient"]) == len(o["gradient"]) and note(tag + " gradient", both(ev["gradient"], o["gradient"])) < TOL
    assert note(tag + " gradient max-norm", rel(ev["gradient_max_norm"], np.abs(o["gradient"]).max())) < TOL
    # the same per family: every gradient entry in units of what it is summed from, residuals and block costs within each factor family
    moved = None
    for fam, v in gradient_error_by_family(ev["gradient"], o).items():
        if note(tag + " gradient / |J|'|r|, " + fam, v) <= GRAD_TOL:
            continue
        assert movement is not None, (tag, fam, v)
        moved = movement() if moved is None else moved
        note(tag + " gradient / |J|'|r|, %s beyond %.0e: the oracle's own movement" % (fam, GRAD_TOL), moved[fam])
        assert v < 30.0 * moved[fam], (tag, fam, v, moved[fam])
    for what, key in (("residuals", "row_family"), ("block costs", "block_family")):
        for fam, v in rel_by_family(ev[what.replace(" ", "_")], o[what.replace(" ", "_")], factor_families(o[key])).items():
            assert note(tag + " %s, %s factors" % (what, fam), v) < TOL, (tag, what, fam, v)


@pytest.fixture(params=["chain", "dense", "cooperative"])
def setting(request, gpu):
    """chain: one workgroup per window; dense: solver variant 1; cooperative: plans chunked for two helper workgroups per window"""
    L = gpu.lib()
    gpu.check(L.tcv_set_solver_variant(1 if request.param == "dense" else 0))
    gpu.check(L.tcv_set_cooperative(2 if request.param == "cooperative" else 0))
    yield request.param
    gpu.check(L.tcv_set_solver_variant(0)); gpu.check(L.tcv_set_cooperative(-1))


def test_parity_against_both_oracles(gpu, setting):
    for name, (w, kw) in cases().items():
        if setting == "dense" and name == "relocalisation":
            continue          # 177 camera tangent dims: the dense layout does not hold such a window (TCV_ERR_TOO_LARGE), tests/test_gpu_relo.py
        exc = not kw.get("estimate_extrinsic", True)
        W, relo = hip_window(gpu, w, **kw)
        b, ev = evaluate_one(gpu, W)
        if setting != "cooperative" or b.cooperative()["helpers"] > 0:
            assert b.plan_stats()["layout"] == ("dense" if setting == "dense" else "chain"), name
        d = b.evaluation_dims(0)
        assert d["num_residuals"] == gpu.lib().tcv_problem_num_residuals(W.h) and d["num_residual_blocks"] == gpu.lib().tcv_problem_num_residual_blocks(W.h)
        assert d["num_local"] == gpu.lib().tcv_problem_num_effective_parameters(W.h)
        o = oracle_evaluate(w, ex_constant=exc)
        check_vs_oracle(ev, o, "numpy oracle:")
        if not any(w.get(k) is not None for k in ("td", "relo")) and not w["line"].get("exact_jacobian"):
            H, g, cost, n, nc = orc.Window(w, ex_constant=exc).linearize_dense()
            assert note("C oracle: cost", rel(ev["cost"], cost)) < TOL and len(g) == len(ev["gradient"])
            assert note("C oracle: gradient", both(ev["gradient"], g)) < TOL
            for fam, v in gradient_error_by_family(ev["gradient"], dict(o, gradient=g)).items():
                assert note("C oracle: gradient / |J|'|r|, " + fam, v) <= GRAD_TOL, (name, fam, v)
        # apply_loss_function = 0 against the oracle on the window without its loss functions
        b.evaluate(apply_loss_function=False, residuals=True, gradient=True, block_costs=True)
        check_vs_oracle(b.evaluation(0), oracle_evaluate(no_loss(w), ex_constant=exc), "numpy oracle, no loss:")


def mixed_batch(n=300):
    batch = synth.make_windows(9400, n)
    wins = []
    for k in range(n):
        w = synth.window_at(batch, k)
        if k % 3 == 1:
            w = dict(w, prior=None)
        if k % 7 == 2:
            w = sub_window(w, 4 + k % 5)
        wins.append(w)
    return wins


def test_mixed_batch_of_300_windows(gpu):
    wins = mixed_batch()
    W = [gpu.Window(w) for w in wins]
    b = gpu.Batch(W)
    assert b.plan_stats()["num_plans"] > 3
    b.evaluate(residuals=True, gradient=True, block_costs=True)
    cost, fam, gmax = b.evaluation_costs()
    assert np.all(np.isfinite(cost)) and np.all(cost > 0) and np.all(gmax > 0)
    assert np.array_equal(cost, ((fam[:, 0] + fam[:, 1]) + fam[:, 2]) + fam[:, 3])
    for k in (0, 1, 2, 9, 151, 298, 299):
        ev = b.evaluation(k)
        assert ev["cost"] == cost[k] and np.array_equal(ev["family_cost"], fam[k]) and ev["gradient_max_norm"] == gmax[k]
        check_vs_oracle(ev, oracle_evaluate(wins[k]), "numpy oracle, batch of 300:")
        b1, ev1 = evaluate_one(gpu, gpu.Window(wins[k]))          # alone (another plan chunking, the whole LDS): the same bits
        for key in ("cost", "family_cost", "gradient_max_norm", "residuals", "block_costs", "gradient"):
            assert np.array_equal(ev[key], ev1[key]), (k, key)


def test_defined_cost_sum_repeatability_and_batch_independence_bit_for_bit(gpu):
    pre, main, z = golden_windows()
    n = 40
    W = [gpu.Window(main) for _ in range(n)]
    b = gpu.Batch(W)
    keys = ("cost", "family_cost", "gradient_max_norm", "residuals", "block_costs", "gradient")
    b.evaluate(residuals=True, gradient=True, block_costs=True)
    first = [b.evaluation(k) for k in range(n)]
    b.evaluate(residuals=True, gradient=True, block_costs=True)
    for k in range(n):
        f = first[k]["family_cost"]
        assert first[k]["cost"] == ((f[0] + f[1]) + f[2]) + f[3]
        again = b.evaluation(k)
        for key in keys:
            assert np.array_equal(first[k][key], again[key]), (k, key)          # two evaluations of one batch
            assert np.array_equal(first[k][key], first[0][key]), (k, key)       # N copies of one window
    b1, alone = evaluate_one(gpu, gpu.Window(main))
    for key in keys:
        assert np.array_equal(alone[key], first[0][key]), key
    b.evaluate()          # cost only: the same costs, no gradient
    c, fam, gmax = b.evaluation_costs()
    assert np.all(c == first[0]["cost"]) and np.all(gmax == -1.0)


def _run(gpu, wins, evaluate):
    W = [gpu.Window(w) for w in wins]
    MW = [gpu.margin_old_window(w) for w in wins]
    M = [gpu.Window(mw, share=W[k], prior=W[k].prior) for k, mw in enumerate(MW)]
    b = gpu.Batch(W, M, [gpu.margin_old_drops(W[k], MW[k]) for k in range(len(wins))])
    ev = []
    if evaluate:
        b.evaluate("initial", residuals=True, gradient=True, block_costs=True)
    b.solve(gpu.default_options(8, True))
    if evaluate:
        b.evaluate("solution", residuals=True, gradient=True, block_costs=True)
    b.gauge_fix(); b.marginalize()
    if evaluate:
        b.evaluate("solution", gradient=True)
    b.synchronize(); b.download_states()
    return W, b.summaries(), [b.prior(k).export() for k in range(len(wins))]


def test_evaluating_does_not_change_what_follows(gpu):
    pre, main, z = golden_windows()
    batch = synth.make_windows(200, 3)
    wins = [main] + [synth.window_at(batch, k) for k in range(3)]
    Wa, sa, pa = _run(gpu, wins, False)
    Wb, sb, pb = _run(gpu, wins, True)
    for k in range(len(wins)):
        for key in ("pose", "sb", "ex", "lam"):
            assert np.array_equal(getattr(Wa[k], key), getattr(Wb[k], key)), (k, key)
        assert sa[k].num_iterations == sb[k].num_iterations and sa[k].termination == sb[k].termination
        assert sa[k].initial_cost == sb[k].initial_cost and sa[k].final_cost == sb[k].final_cost
        assert list(sa[k].cost) == list(sb[k].cost) and list(sa[k].step_norm) == list(sb[k].step_norm)
        assert np.array_equal(pa[k]["J0"], pb[k]["J0"]) and np.array_equal(pa[k]["r0"], pb[k]["r0"])
        assert all(np.array_equal(a, c) for a, c in zip(pa[k]["x0"], pb[k]["x0"]))


def test_consistency_with_the_solver_and_the_gauge_fixed_states(gpu):
    pre, main, z = golden_windows()
    wins = [pre, main, synth.window_at(synth.make_windows(200, 1), 0)]
    for fused in (False, True):
        W = [gpu.Window(w) for w in wins]
        b = gpu.Batch(W)
        if fused:
            b.fuse_gauge_fix()
        b.evaluate("initial")
        c0 = b.evaluation_costs()[0]
        b.solve(gpu.default_options(8, True))
        b.evaluate("solution", residuals=True, gradient=True, block_costs=True)
        c1 = b.evaluation_costs()[0]
        b.download_states()
        s = b.summaries()
        for k, w in enumerate(wins):
            assert note("solver: initial_cost", rel(c0[k], s[k].initial_cost)) < TOL
            if not fused:
                assert note("solver: final_cost", rel(c1[k], s[k].final_cost)) < TOL
            x = oracle_state(NO.Problem(w), W[k])
            o = oracle_evaluate(w, x)
            check_vs_oracle(b.evaluation(k), o, "numpy oracle at the %s states:" % ("gauge-fixed" if fused else "solved"), lambda: oracle_gradient_movement(w, x, o))


def test_problem_evaluate_at_the_callers_current_values(gpu):
    w = synth.window_at(synth.make_windows(700, 1), 0)
    W = gpu.Window(w)
    before = W.states()
    pe = W.evaluate()
    b, ev = evaluate_one(gpu, W)
    assert pe["cost"] == ev["cost"] and np.array_equal(pe["family_cost"], ev["family_cost"])
    assert np.array_equal(pe["residuals"], ev["residuals"]) and np.array_equal(pe["gradient"], ev["gradient"])
    for k, v in before.items():
        assert np.array_equal(v, W.states()[k])
    assert W.evaluate(residuals=False, gradient=False)["cost"] == pe["cost"]
    s = gpu.SolverSummary(); o = gpu.default_options(8, True)
    gpu.check(gpu.lib().tcv_solve(C.byref(o), W.h, C.byref(s)))
    solved = W.states()
    pe = W.evaluate()
    assert note("problem_evaluate: final_cost", rel(pe["cost"], s.final_cost)) < TOL
    oe = oracle_evaluate(w, oracle_state(NO.Problem(w), W))
    assert note("problem_evaluate: cost", rel(pe["cost"], oe["cost"])) < TOL
    assert note("problem_evaluate: residuals", both(pe["residuals"], oe["residuals"])) < TOL
    assert note("problem_evaluate: gradient", both(pe["gradient"], oe["gradient"])) < TOL
    for fam, v in gradient_error_by_family(pe["gradient"], oe).items():
        assert note("problem_evaluate: gradient / |J|'|r|, " + fam, v) <= GRAD_TOL, (fam, v)
    for k, v in solved.items():
        assert np.array_equal(v, W.states()[k])
    W.evaluate(apply_loss_function=False)


def test_directional_derivative_pin(gpu):
    """(cost(x + eps d) - cost(x - eps d)) / 2 eps against g . d through tcv_problem_evaluate at perturbed caller states, on windows
    whose Jacobian is the derivative of their residual (no line factors, or line_exact_jacobian = 1; include/tcv.h
    tcv_problem_set_line_jacobian).  Gate: 10 x the worst figure the NumPy oracle's own g and cost show for the same windows and seeds."""
    cs = cases()
    for name in ("synth_points_only", "line_exact"):
        w, kw = cs[name]
        P = NO.Problem(w)
        x0 = P.x0()
        J, r, c = P.linearize(x0)
        g_o = J.T @ r
        W, _ = hip_window(gpu, w, **kw)
        g_d = W.evaluate(residuals=False)["gradient"]

        def dev_cost(x):
            W.pose[:] = x["pose"]; W.sb[:] = x["sb"]; W.ex[:] = x["ex"]; W.lam[:] = x["lam"]
            return W.evaluate(residuals=False, gradient=False)["cost"]
        worst_o = worst_d = 0.0
        for seed in range(4):
            d = np.random.default_rng(1000 + seed).normal(size=P.nlocal)
            d /= np.linalg.norm(d)
            worst_o = max(worst_o, directional_error(lambda x: P.linearize(x, want_jac=False)[2], g_o, P.plus, x0, d))
            worst_d = max(worst_d, directional_error(dev_cost, g_d, P.plus, x0, d))
        dev_cost(x0)
        print("directional derivative, %s: oracle %.3e, device %.3e" % (name, worst_o, worst_d))
        note("directional derivative (%s): oracle" % name, worst_o); note("directional derivative (%s): device" % name, worst_d)
        assert worst_d < 10.0 * worst_o, name


def test_argument_validation_on_a_resident_batch(gpu):
    L = gpu.lib()
    W = gpu.Window(synth.window_at(synth.make_windows(5, 1), 0))
    b = gpu.Batch([W])
    d = np.zeros(4096)
    o = gpu.evaluate_options("solution")
    assert L.tcv_batch_evaluate(b.h, C.byref(o), None) == gpu.TCV_ERR_INVALID and b"not been solved" in L.tcv_last_error()
    assert L.tcv_batch_get_evaluation_costs(b.h, gpu.dptr(d), None, None, 1) == gpu.TCV_ERR_INVALID          # nothing evaluated yet
    o.at = 5
    assert L.tcv_batch_evaluate(b.h, C.byref(o), None) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_evaluate(b.h, None, None) == gpu.TCV_ERR_INVALID
    b.evaluate(residuals=True)
    dims = b.evaluation_dims(0)
    for win in (-1, 1):
        assert L.tcv_batch_evaluation_dims(b.h, win, None, None, None) == gpu.TCV_ERR_INVALID
        assert L.tcv_batch_get_evaluation(b.h, win, gpu.dptr(d), None, None, None, 0, None, 0, None, 0) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_get_evaluation(b.h, 0, gpu.dptr(d), None, None, gpu.dptr(d), dims["num_residuals"] - 1, None, 0, None, 0) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_get_evaluation(b.h, 0, gpu.dptr(d), None, None, None, 0, None, 0, gpu.dptr(d), 4096) == gpu.TCV_ERR_INVALID and b"not asked for" in L.tcv_last_error()
    assert L.tcv_batch_get_evaluation(b.h, 0, gpu.dptr(d), None, None, None, 0, gpu.dptr(d), 4096, None, 0) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_get_evaluation_costs(b.h, gpu.dptr(d), None, None, 2) == gpu.TCV_ERR_INVALID
    c = np.zeros(1)
    assert L.tcv_batch_get_evaluation(b.h, 0, gpu.dptr(c), None, None, gpu.dptr(d), dims["num_residuals"], None, 0, None, 0) == gpu.TCV_OK
    assert c[0] == b.evaluation(0)["cost"] and np.array_equal(d[:dims["num_residuals"]], b.evaluation(0)["residuals"])
    b.evaluate(stream=gpu.STREAM_THREAD)          # the calling thread's own stream
    assert b.evaluation(0)["cost"] == c[0]
    # NaN in the evaluation point: TCV_ERR_NUMERIC, nothing aborts
    w = synth.window_at(synth.make_windows(5, 1), 0)
    W2 = gpu.Window(w); b2 = gpu.Batch([W2])
    b2.solve(gpu.default_options(0, True)); b2.synchronize()
    W2.lam[0] = 0.0          # 1 / inverse depth
    with pytest.raises(gpu.TcvError) as e:
        W2.evaluate()
    assert e.value.status == gpu.TCV_ERR_NUMERIC


def test_evaluation_buffers_go_back_with_the_batch(gpu):
    W = [gpu.Window(synth.window_at(synth.make_windows(5, 2), k)) for k in range(2)]
    live0 = gpu.device_memory_stats()[0]
    b = gpu.Batch(W)
    live1 = gpu.device_memory_stats()[0]
    b.evaluate(residuals=True, gradient=True, block_costs=True); b.evaluation(1)
    assert gpu.device_memory_stats()[0] > live1
    b.solve(gpu.default_options(2, True)); b.evaluate("solution"); b.synchronize()
    gpu.lib().tcv_batch_destroy(b.h); b.h = None
    assert gpu.device_memory_stats()[0] == live0
    W[0].evaluate()
    assert gpu.device_memory_stats()[0] == live0


def test_ceres_shim_problem_evaluate(gpu, tmp_path):
    """include/tcv_ceres_shim.hpp Problem::Evaluate, compiled and run the way tests/test_gpu_solve.py runs the C++ callers"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.LIB_PATH)
    exe = os.path.join(tmp_path, "estimator_shim_classes")
    subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "estimator_shim_classes.cpp"), "-L" + libdir, "-ltcv_hip",
                           "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ev = re.findall(r"evaluate \((before|after)\): cost (\S+) = prior (\S+) \+ imu (\S+) \+ points (\S+) \+ lines (\S+); (\d+) residuals, (\d+) gradient entries", r.stdout)
    assert [e[0] for e in ev] == ["before", "after"], r.stdout
    sv = re.search(r"solve: (\d+) iterations, cost (\S+) -> (\S+), inverse depth (\S+)", r.stdout).groups()
    assert abs(float(ev[0][1]) - float(sv[1])) < 1e-5 * float(sv[1])          # (the summary line is printed with six digits)
    assert float(ev[1][1]) < 1e-9 * float(ev[0][1])          # the toy window is solved to round-off: only the magnitude is comparable
    for e in ev:
        assert float(e[1]) == ((float(e[2]) + float(e[3])) + float(e[4])) + float(e[5])
    assert int(ev[0][6]) > 0 and int(ev[0][7]) > 0


def test_zz_report():
    for k in sorted(WORST):
        print("worst %-100s %.3e" % (k, WORST[k]))
