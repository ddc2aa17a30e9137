"""CPU side of the batched 4-DoF pose-graph optimisation (include/tcv_pose_graph.h): the NumPy restatement (tests/pose_graph_oracle.py)
against central differences and against scipy's least squares on the same cost, the input validation of the C-ABI (which runs before the
device is touched), the loud failure without a device, the header as C99 / C++14, and the host-side elimination order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_graph_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tcv_pose_graph.h")


@pytest.fixture(scope="module")
def pg(built):
    import tcv_pose_graph
    return tcv_pose_graph


def test_oracle_jacobians_against_central_differences():
    rng = np.random.default_rng(1)
    worst = 0.0
    for n in range(60):
        kind, xi, xj, meas = PO.random_edge(rng, n % 2, big_tilt=n % 3 == 0, huber=[None, True, False][n % 3])
        _, r, Ji, Jj = PO.edge(kind, xi, xj, meas, correct=False)
        for J, which in ((Ji, 0), (Jj, 1)):
            for k in range(4):
                h = 1e-6
                xp, xm = [xi.copy(), xj.copy()], [xi.copy(), xj.copy()]
                xp[which][k] += h; xm[which][k] -= h
                num = (PO.edge(kind, xp[0], xp[1], meas, correct=False)[1] - PO.edge(kind, xm[0], xm[1], meas, correct=False)[1]) / (2 * h)
                worst = max(worst, float(np.abs(num - J[:, k]).max()))
    assert worst < 1e-7, worst      # central differences at h = 1e-6 on values of order 1..10: truncation + rounding ~1e-9


def test_oracle_corrector_matches_the_huber_cost():
    """the corrected residual of an active Huber edge has |r_c|^2 = rho' |r|^2, the cost is rho / 2; inactive edges are untouched"""
    rng = np.random.default_rng(2)
    active = 0
    for n in range(40):
        kind, xi, xj, meas = PO.random_edge(rng, 1, huber=bool(n % 2))
        cost, rc, _, _ = PO.edge(kind, xi, xj, meas)
        _, r, _, _ = PO.edge(kind, xi, xj, meas, correct=False)
        s = float(r @ r)
        if s > 0.01:
            active += 1
            assert np.isclose(cost, 0.5 * (0.2 * np.sqrt(s) - 0.01), rtol=1e-14) and np.isclose(float(rc @ rc), 0.1 / np.sqrt(s) * s, rtol=1e-13)
        else:
            assert cost == 0.5 * s and np.array_equal(r, rc)
    assert 10 <= active <= 30


def test_oracle_minimum_against_scipy_least_squares():
    so = pytest.importorskip("scipy.optimize")
    for name in ("n6", "n12_const_and_free_old", "n12_huber", "n20_sequences"):
        g = PO.test_graphs()[name]
        ref = PO.solve(g, opt=dict(max_num_iterations=200), ceres=dict(function_tolerance=1e-15, parameter_tolerance=1e-14))
        G = PO.Graph(g)
        x0 = G.x0()

        def residuals(v):
            x = x0.copy()
            x[G.free] = v.reshape(-1, 4)
            out = []
            for (k, a, b, m) in G.red:
                cost, r, _, _ = PO.edge(k, x[a], x[b], m, G.opt, correct=False, want_jac=False)
                n = np.linalg.norm(r)
                out.append(r * (np.sqrt(2 * cost) / n if n > 0 else 1.0))      # |out|^2 / 2 = rho / 2
            return np.concatenate(out)

        res = so.least_squares(residuals, x0[G.free].ravel(), xtol=1e-15, ftol=1e-15, gtol=1e-15)
        fixed = G.cost(x0, G.fixed)
        assert abs(res.cost + fixed - ref["summary"]["final_cost"]) <= 1e-8 * max(1e-3, res.cost), (name, res.cost + fixed, ref["summary"]["final_cost"])
        assert np.abs(res.x.reshape(-1, 4) - ref["x"][G.free]).max() < 1e-4, name


def test_oracle_reaches_every_path_the_gpu_tests_rely_on():
    G = PO.test_graphs()
    codes = {k: PO.solve(g)["summary"]["termination"] for k, g in G.items()}
    assert codes["n1"] == "CONVERGENCE_GRADIENT" and codes["n12_no_loops"] == "CONVERGENCE_GRADIENT"
    assert "CONVERGENCE_FUNCTION" in codes.values() and "NO_CONVERGENCE" in codes.values()
    assert PO.CERES_DEFAULTS["initial_trust_region_radius"] == 1e4 and PO.REFERENCE_OPTIONS["max_num_iterations"] == 5


def test_header_functions_are_exported_and_mirrored(pg):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(tcv_pose_graphs?_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 5, declared
    L = pg.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"libtcv_hip.so does not export {name}"
    assert declared == set(pg.EXPORTS)
    import tcv
    assert not any(n.startswith("tcv_pose_graph") for n in tcv.EXPORTS)
    assert "tcv_pose_graph" not in open(os.path.join(ROOT, "include", "tcv.h")).read()
    assert "tcv_pose_graph" not in open(os.path.join(ROOT, "include", "tcv_estimator.h")).read()
    src = open(os.path.join(ROOT, "tc-viml_amd", "tcv_pose_graph.py")).read()
    assert "pose_graph_oracle" not in src and "np_oracle" not in src and "import orc" not in src
    for k, v in (("MAX_NODES", pg.MAX_NODES), ("MAX_LOOPS", pg.MAX_LOOPS), ("MAX_BATCH", pg.MAX_BATCH), ("MAX_TRACE", pg.MAX_TRACE)):
        assert re.search(r"#define TCV_POSE_GRAPH_%s %d\b" % (k, v), hdr), k
    assert pg.MAX_NODES >= 2048 and pg.MAX_LOOPS >= 256


def test_header_is_valid_c99_and_cxx14(pg, tmp_path):
    c = os.path.join(tmp_path, "t.c")
    open(c, "w").write('#include "tcv_pose_graph.h"\nint main(void){ tcv_pose_graph_options o; tcv_pose_graph_options_default(&o); '
                       'return (int)sizeof(tcv_pose_graph_summary) > 0 && sizeof(tcv_pose_graph_desc) > 0 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + inc, "-fsyntax-only", c])
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + inc, "-x", "c++", "-fsyntax-only", c])
    # the mirror's structures have the header's sizes: a C program prints them
    exe = os.path.join(tmp_path, "sizes")
    open(c, "w").write('#include <stdio.h>\n#include "tcv_pose_graph.h"\nint main(void){ printf("%d %d %d\\n", (int)sizeof(tcv_pose_graph_desc), '
                       '(int)sizeof(tcv_pose_graph_options), (int)sizeof(tcv_pose_graph_summary)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I" + inc, c, "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(pg.Desc), C.sizeof(pg.Options), C.sizeof(pg.Summary)]


def test_defaults_reproduce_the_reference(pg):
    o = pg.default_options()
    assert (o.max_num_iterations, o.huber_delta, o.loop_weight, o.loop_yaw_divisor) == (5, 0.1, 1.0, 10.0)
    D = PO.CERES_DEFAULTS
    assert (o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius, o.min_relative_decrease) == \
        (D["function_tolerance"], D["gradient_tolerance"], D["parameter_tolerance"], D["initial_trust_region_radius"], D["min_relative_decrease"])


def test_every_validation_error(pg):
    import tcv
    L = pg.lib()
    good = PO.test_graphs()["n12_const_and_free_old"]

    def rc_of(edit=None, **kw):
        g = pg.Graph({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in dict(good, **kw).items()})      # (copies: the edits poke)
        if edit:
            edit(g)
        return pg.optimize_raw([g.desc])[0]

    def setf(**f):
        def e(g):
            for k, v in f.items():
                setattr(g.desc, k, v)
        return e

    def poke(arr, idx, val):
        def e(g):
            getattr(g, arr).reshape(-1)[idx] = val
        return e

    INV = tcv.TCV_ERR_INVALID
    assert rc_of(setf(n_nodes=0)) == INV and b"n_nodes" in L.tcv_last_error()
    assert rc_of(setf(t=None)) == INV and b"missing array" in L.tcv_last_error()
    assert rc_of(setf(q_xyzw=None)) == INV
    assert rc_of(setf(n_loops=-1)) == INV
    for f in ("loop_cur", "loop_old", "loop_relative_t", "loop_relative_yaw"):
        assert rc_of(setf(**{f: None})) == INV and b"missing array" in L.tcv_last_error(), f
    assert rc_of(poke("cur", 0, 12)) == INV and b"out of range" in L.tcv_last_error()
    assert rc_of(poke("old", 1, -1)) == INV and b"out of range" in L.tcv_last_error()
    assert rc_of(poke("old", 1, 10)) == INV and b"loop_old >= loop_cur" in L.tcv_last_error()
    assert rc_of(poke("old", 1, 11)) == INV
    for arr, val in (("t", np.nan), ("q", np.inf), ("rel_t", np.nan), ("rel_yaw", -np.inf)):
        assert rc_of(poke(arr, 1, val)) == INV and b"non-finite" in L.tcv_last_error(), arr
    assert rc_of(q=np.zeros((12, 4))) == INV and b"zero quaternion" in L.tcv_last_error()
    # the call's own arguments
    g = pg.Graph(good)
    arr = (pg.Desc * 1)(g.desc)
    sums = (pg.Summary * 1)()
    assert L.tcv_pose_graphs_optimize(0, arr, None, None, None, sums, None) == INV
    assert L.tcv_pose_graphs_optimize(1, None, None, None, None, sums, None) == INV
    assert L.tcv_pose_graphs_optimize(1, arr, None, None, None, None, None) == INV
    assert pg.optimize_raw([g.desc], pg.default_options(initial_trust_region_radius=0.0))[0] == INV
    assert pg.optimize_raw([g.desc], pg.default_options(huber_delta=np.nan))[0] == INV
    # the second graph of a batch is validated too
    bad = pg.Graph(dict(good)); bad.desc.t = None
    assert pg.optimize_raw([g.desc, bad.desc])[0] == INV and b"pose graph 1" in L.tcv_last_error()
    # edges
    with pytest.raises(tcv.TcvError) as e:
        pg.eval_edges([2], [0.0], np.zeros(3), [0.0], np.zeros(3), np.zeros(6))
    assert e.value.status == INV
    with pytest.raises(tcv.TcvError) as e:
        pg.eval_edges([0], [np.nan], np.zeros(3), [0.0], np.zeros(3), np.zeros(6))
    assert e.value.status == INV
    assert L.tcv_pose_graph_plan_stats(None, None, None) == INV


def test_limits_are_unsupported_before_any_launch(pg):
    """beyond the declared limits: TCV_ERR_UNSUPPORTED, with or without a device (the check sits in front of the device test)"""
    import tcv
    n = pg.MAX_NODES + 1
    q = np.tile([0.0, 0, 0, 1], (n, 1))
    big = dict(t=np.zeros((n, 3)), q=q, loops=[])
    gb = pg.Graph(big)      # (a Graph keeps the arrays behind its descriptor alive)
    assert pg.optimize_raw([gb.desc])[0] == tcv.TCV_ERR_UNSUPPORTED and b"TCV_POSE_GRAPH_MAX_NODES" in pg.lib().tcv_last_error()
    n = 600
    many = dict(t=np.zeros((n, 3)), q=np.tile([0.0, 0, 0, 1], (n, 1)), loops=[(300 + k, k, np.zeros(3), 0.0) for k in range(pg.MAX_LOOPS + 1)])
    gm = pg.Graph(many)
    assert pg.optimize_raw([gm.desc])[0] == tcv.TCV_ERR_UNSUPPORTED
    ok = pg.Graph(PO.test_graphs()["n5"])
    assert pg.optimize_raw([ok.desc, gb.desc])[0] == tcv.TCV_ERR_UNSUPPORTED


def test_valid_input_without_a_device_is_no_device(pg):
    import tcv
    if tcv.lib().tcv_device_count() > 0:
        pytest.skip("a HIP device is visible")
    g = PO.test_graphs()["n12_const_and_free_old"]
    with pytest.raises(tcv.TcvError) as e:
        pg.optimize([g])
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE
    with pytest.raises(tcv.TcvError) as e:
        pg.eval_edges([0], [0.0], np.zeros(3), [1.0], np.ones(3), np.zeros(6))
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE


def test_elimination_order_band_and_border(pg):
    G = PO.test_graphs()
    expect = {      # name: (free, band, border, reduced edges, fixed edges)
        "n1": (0, 0, 0, 0, 0),
        "n2": (1, 1, 0, 2, 0),                              # the loop's older end is the constant node 0: no border
        "n5": (4, 3, 1, 10 + 1, 0),
        "n6": (5, 4, 1, 14 + 1, 0),
        "n12_const_and_free_old": (11, 10, 1, 38 + 2, 0),    # (11 -> 0) has a constant older end, (10 -> 2) makes node 10 a border node
        "n12_loop_in_band": (11, 10, 1, 38 + 1, 0),
        "n16_consecutive_borders": (15, 11, 4, 54 + 4, 0),
        "n16_shared_newer": (15, 14, 1, 54 + 2, 0),
        "n12_no_loops": (11, 11, 0, 38, 0),
    }
    for name, (free, band, border, edges, fixed) in expect.items():
        st = pg.plan_stats(G[name])
        assert (st["free"], st["band"], st["border"], st["edges"], st["fixed_edges"]) == (free, band, border, edges, fixed), (name, st)
        assert st["half_bandwidth"] == 19
        ref = PO.Graph(G[name])
        assert st["free"] == len(ref.free) and st["edges"] == len(ref.red) and st["fixed_edges"] == len(ref.fixed)
    # positions: constants -1, band in keyframe order, then the border in keyframe order
    st = pg.plan_stats(G["n16_consecutive_borders"])
    assert list(st["position"]) == [-1] + list(range(11)) + [11, 12, 13, 14]
    # sequence 0 prefix (constant), a sequence change in the middle: nodes 0..3 constant, their six mutual edges and the loop (3 -> 1) fixed
    st = pg.plan_stats(G["n20_sequences"])
    ref = PO.Graph(G["n20_sequences"])
    assert list(np.where(st["position"] < 0)[0]) == [0, 1, 2, 3] and st["fixed_edges"] == 7 == len(ref.fixed) and st["border"] == 2
    st = pg.plan_stats(G["n300"])
    assert st["border"] == 40 and st["band"] == 259 and st["scratch_bytes"] < 4 << 20


# ------------------------------------------------------------------------- what the boundary and fuzz tests of the GPU suite rest on
MARGIN = 0.01      # derived, not measured: the GPU file's relative cost gate (2.3e-13) moves a cost-change ratio next to the 1e-6 function tolerance
#                    by at most about 5e-7 relative, and every other decision by less; 1 % is 2e4 times that


def test_boundary_graphs_have_the_intended_shapes(pg):
    """the table of pose_graph_oracle.BOUNDARY_SHAPES is only worth something if the host's order really produces these shapes"""
    G = PO.boundary_graphs()
    assert len(G) == len(PO.BOUNDARY_SHAPES) == 25
    for (nb, nk), (name, g) in zip(PO.BOUNDARY_SHAPES, G.items()):
        st = pg.plan_stats(g)
        assert (st["free"], st["band"], st["border"]) == (nb + nk, nb, nk), (name, st)
        assert len(g["t"]) == 1 + nb + nk and len(g["loops"]) <= pg.MAX_LOOPS
    sizes = {(4 * nb, 4 * nk) for nb, nk in PO.BOUNDARY_SHAPES}
    assert {nbs for nbs, _ in sizes} >= {4, 8, 16, 20, 24, 32, 36, 300, 304, 320, 324, 600, 604}
    assert {m for _, m in sizes} >= {4, 60, 64, 68, 252, 256, 260, 512, 1024}


def test_boundary_graphs_decide_clear_of_every_threshold():
    """every comparison of the oracle's loop at least 1 % from its threshold, so that the device may not legitimately decide otherwise;
    no invalid step; a graph that fails this gets another seed in pose_graph_oracle.BOUNDARY_SEEDS, none is skipped on the GPU"""
    for name, g in PO.boundary_graphs().items():
        s = PO.solve(g)["summary"]
        margin, what, record = PO.decision_margin(s)
        print("%-10s records %d %-22s margin %.3g (%s, record %d)" % (name, len(s["iterations"]), s["termination"], margin, what, record))
        assert all(i["step"] >= 0 for i in s["iterations"]) and 2 <= len(s["iterations"]) <= 6, name
        assert s["termination"] in ("CONVERGENCE_FUNCTION", "CONVERGENCE_PARAMETER", "NO_CONVERGENCE"), (name, s["termination"])
        assert margin >= MARGIN, (name, margin, what, record)


def test_decision_margin_sees_each_threshold():
    """decision_margin on records made by hand: each comparison is found, in the loop's order, and not past the one that ended the solve"""
    first = dict(cost=1.0, cost_candidate=0.0, rho=0.0, radius=1e4, step=1, gradient_max=1.0)
    rec = dict(cost=0.5, cost_candidate=0.5, rho=0.9, radius=1e4, step=1, model_cost_change=0.55, step_norm=1.0, x_norm=10.0, gradient_max=1.0)
    S = lambda *its, term="NO_CONVERGENCE": dict(iterations=list(its), termination=term)
    assert PO.decision_margin(S(first, rec))[0] > 0.99
    assert PO.decision_margin(S(dict(first, gradient_max=1.005e-10)))[:2] == (pytest.approx(0.005), "gradient_tolerance")
    assert PO.decision_margin(S(first, dict(rec, gradient_max=0.998e-10)))[1:] == ("gradient_tolerance", 1)
    assert PO.decision_margin(S(first, dict(rec, rho=1.003e-3)))[:2] == (pytest.approx(0.003), "min_relative_decrease")
    assert PO.decision_margin(S(first, dict(rec, cost_candidate=1.0 - 1.004e-6)))[:2] == (pytest.approx(0.004, rel=1e-3), "function_tolerance")
    assert PO.decision_margin(S(first, dict(rec, step_norm=1.002e-7)))[:2] == (pytest.approx(0.002, rel=1e-3), "parameter_tolerance")
    # a rejected record carries the unchanged cost; the record that ends on the function tolerance is not asked for its rho
    end = dict(rec, cost=1.0, cost_candidate=1.0 - 0.5e-6, rho=1.0001e-3, step=0)
    assert PO.decision_margin(S(first, end, term="CONVERGENCE_FUNCTION"))[:2] == (pytest.approx(0.5, rel=1e-3), "function_tolerance")
    assert PO.decision_margin(S(first, dict(end, step=-1)))[0] == 0.0


def test_fuzz_population_decides_clear_of_the_thresholds():
    """tests/dev/fuzz_pose_graph.py over the seed range of its GPU gate (tests/test_gpu_fuzz.py), the oracle alone: at most 2 % of the cases
    within 1 % of a threshold (those the fuzzer lists and skips), every termination it claims to cover present, no invalid step"""
    import sys
    dev = os.path.join(ROOT, "tests", "dev")
    sys.path.insert(0, dev)
    try:
        import fuzz_pose_graph as F
    finally:
        sys.path.remove(dev)
    assert (F.MARGIN, F.MAX_SKIPPED) == (MARGIN, 0.02)
    pop = F.population(200, 0)
    close = [(seed, what, m) for seed, _, what, _, m in pop if m[0] < MARGIN]
    tally = {}
    for c in pop:
        tally[c[3]["summary"]["termination"]] = tally.get(c[3]["summary"]["termination"], 0) + 1
    print("terminations:", tally, " within the band:", close)
    assert len(close) <= 0.02 * len(pop), close
    assert not any(i["step"] < 0 for c in pop for i in c[3]["summary"]["iterations"])
    assert all(tally.get(k, 0) >= 10 for k in ("CONVERGENCE_GRADIENT", "CONVERGENCE_FUNCTION", "CONVERGENCE_PARAMETER", "NO_CONVERGENCE")), tally
    shapes = [(len(c[3]["summary"]["iterations"]), c[3]["summary"]["num_free_nodes"]) for c in pop]
    assert max(f for _, f in shapes) >= 100 and min(f for _, f in shapes) <= 1
