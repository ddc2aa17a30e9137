"""Batched 4-DoF pose-graph optimisation on the device (include/tcv_pose_graph.h, csrc/tcv_pose_graph.hip) against its NumPy restatement
(tests/pose_graph_oracle.py): the edge maths on seeded edges, every graph of pose_graph_oracle.test_graphs() solved once alone and once
in one ragged batch, every termination and step path (asserted on the ORACLE's trace first, so that no test passes vacuously), bit-exact
determinism, the limits and the drift.

Gates.  Traces (records, accepted / rejected per record, termination code) must be identical.  Every numerical gate is three times the
worst figure measured on an MI355X over all tests of this file (profiles/pose_graph.txt has the table per graph); none on a state is
looser than the project's 1e-6 criterion:
    edge residual / Jacobian / cost, absolute    measured 4.4e-16 / 1.2e-15 / 3.3e-16   gate 4e-15 (three times the largest)
    costs of the trace, relative                 measured 7.6e-14 (n20_sequences)       gate 2.3e-13
    rho of the trace, absolute                   measured 2.3e-7  (n12_loop_in_band)    gate 7e-7
    positions, absolute (metres)                 measured 3.6e-14 (n300)                gate 1.1e-13
    rotations and r_drift, matrix entries        measured 1.3e-15 (n300)                gate 4e-15
    yaw_drift (degrees) / t_drift (metres)       measured 1.4e-14 / 3.2e-14             gate 4.3e-14 / 9.6e-14
rho of the record that ends a solve on the function tolerance divides a cost change of <= 1e-6 of the cost by a model change of the same
size: the relative rounding of the two costs (1e-14) arrives there multiplied by 1e6 and more.  Every other rho agrees to 1.5e-11.

The boundary sweep (pose_graph_oracle.boundary_graphs(): a graph on and next to every size built into the kernel) and the structure fuzzer
(tests/dev/fuzz_pose_graph.py, gated from tests/test_gpu_fuzz.py) use the same constants wherever their measured worst stays inside them;
where a shape legitimately exceeds one, that test has its own gate of three times its own measured worst (profiles/pose_graph.txt, per graph):
    boundary  rho of the ending record          measured 3.3e-5  (b4_k0)     gate 9.8e-5     cost / model change 9.5e10 there, cond x eps 1.2e-15
              rho of every other record         measured 1.5e-9  (b80_k0)    gate 7e-7 (the file's)
              yaw_drift / t_drift               measured 8.5e-14 / 1.5e-13 (b8_k256, 1024 border unknowns)   gate 2.6e-13 / 4.4e-13
    fuzz      costs of the trace, relative      measured 2.1e-7  (seed 10)   gate 6.3e-7     a single exact loop: the cost falls to 4e-20
              rho of the ending record          measured 8.5e-3  (seed 17)   gate 2.6e-2     cost / model change 1.4e11 there
              rho of every other record         measured 4.2e-9  (seed 32)   gate 7e-7 (the file's)
              positions / rotations, r_drift    measured 4.3e-11 (seed 42) / 1.9e-12 (seed 37)      gate 1.3e-10 / 5.7e-12, 5.4e-12
              yaw_drift / t_drift               measured 1.1e-10 (seed 37) / 5.2e-11 (seed 42)      gate 3.3e-10 / 1.5e-10
The fuzz figures on states are 1e3 times the table's: those are graphs whose only tie to a constant node is a grossly wrong loop that
the Huber loss has switched down, at a radius of 8e5, and the oracle's damped normal matrix has cond x eps of 1.2e-11 (seed 37), 4.3e-11
(seed 42) against 1e-12 for n300; the error of a state is that times its size (180 degrees, 30 metres).  All are far inside the 1e-6 criterion.
The record past the cap (test_trace_longer_than_the_record_cap) gates rho per record by propagation instead: steps at a radius of 1e-8
change the cost by 1e-9 of itself, so the bound is 2 GATE_COST_REL cost / |model change| + 3 x 1.5e-11; measured 1.8e-6 at a bound of 6e-4
(n20_sequences, record 1), 1.4e-13 at 1.9e-10 (record 15)."""
import functools

import numpy as np
import pytest

import pose_graph_oracle as PO

pytestmark = pytest.mark.gpu

GATE_EDGE = 4e-15
GATE_COST_REL = 2.3e-13
GATE_RHO = 7e-7
GATE_T = 1.1e-13
GATE_R = 4e-15
GATE_YAW_DRIFT = 4.3e-14
GATE_T_DRIFT = 9.6e-14
FILE_GATES = dict(cost_rel=GATE_COST_REL, rho=GATE_RHO, rho_before_end=GATE_RHO, t=GATE_T, R=GATE_R, yaw_drift=GATE_YAW_DRIFT, t_drift=GATE_T_DRIFT, r_drift=GATE_R)
# the boundary sweep and the structure fuzzer: the constants above wherever their measured worst stays inside them, three times their own
# measured worst where a shape legitimately exceeds one (the docstring says which and why)
BOUNDARY_GATES = dict(FILE_GATES, rho=9.8e-5, yaw_drift=2.6e-13, t_drift=4.4e-13)
FUZZ_GATES = dict(FILE_GATES, cost_rel=6.3e-7, rho=2.6e-2, t=1.3e-10, R=5.7e-12, yaw_drift=3.3e-10, t_drift=1.5e-10, r_drift=5.4e-12)


@pytest.fixture(scope="module")
def pg(gpu):
    import tcv_pose_graph
    return tcv_pose_graph


@functools.lru_cache(maxsize=None)
def graphs():
    return PO.test_graphs()


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's answer for every test graph at the reference's options: made once, shared, never changed"""
    return {k: PO.solve(g) for k, g in graphs().items()}


_device = {}


def device(pg):
    """every graph solved alone, and all of them in one batch: made once"""
    if not _device:
        names = list(graphs())
        _device["solo"] = {k: pg.optimize([graphs()[k]])[0] for k in names}
        _device["batch"] = dict(zip(names, pg.optimize([graphs()[k] for k in names])))
    return _device


def trace_of(summary):
    """(number of records, step per record, termination code) of an oracle or a device summary"""
    if isinstance(summary["iterations"], int):
        return summary["iterations"], list(summary["step"]), summary["termination"]
    return len(summary["iterations"]), [i["step"] for i in summary["iterations"]], summary["termination_code"]


def compare(dev, ref, figures):
    """traces identical; the numerical differences go into `figures` (max per kind)"""
    s, so = dev["summary"], ref["summary"]
    assert trace_of(s) == trace_of(so), (trace_of(s), trace_of(so))
    assert (s["num_free_nodes"], s["num_edges"]) == (so["num_free_nodes"], so["num_edges"])
    n = len(so["iterations"])
    assert np.all(np.isfinite(dev["t"])) and np.all(np.isfinite(dev["R"]))

    def upd(k, v):
        figures[k] = max(figures.get(k, 0.0), float(v))

    for key in ("cost", "cost_candidate"):
        a = np.array([i[key] for i in so["iterations"]]); b = s[key][:n]
        upd("cost_rel", np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300) * (np.abs(a) > 1e-20)))
    for key in ("initial_cost", "final_cost"):
        if abs(so[key]) > 1e-20:
            upd("cost_rel", abs(s[key] - so[key]) / abs(so[key]))
    d_rho = np.abs(np.array([i["rho"] for i in so["iterations"]]) - s["rho"][:n])
    upd("rho", np.max(d_rho))
    ends_on_a_tolerance = so["termination"] in ("CONVERGENCE_FUNCTION", "CONVERGENCE_PARAMETER")      # (the record whose rho divides a vanishing cost change)
    upd("rho_before_end", np.max(d_rho[:n - 1]) if ends_on_a_tolerance and n > 1 else np.max(d_rho))
    assert np.allclose([i["radius"] for i in so["iterations"]], s["radius"][:n], rtol=1e-9, atol=0)      # a function of the accepted steps' rho (>= 1e-11 apart), cubed
    upd("t", np.max(np.abs(dev["t"] - ref["t"])))
    upd("R", np.max(np.abs(dev["R"] - ref["R"])))
    upd("yaw_drift", abs(s["yaw_drift"] - so["yaw_drift"]))
    upd("t_drift", np.max(np.abs(s["t_drift"] - so["t_drift"])))
    upd("r_drift", np.max(np.abs(s["r_drift"] - so["r_drift"])))


def gate(figures, quiet=False):
    if not quiet:
        print("measured:", {k: "%.3g" % v for k, v in figures.items()})
    assert figures.get("cost_rel", 0) <= GATE_COST_REL and figures.get("rho", 0) <= GATE_RHO, figures
    assert figures.get("t", 0) <= GATE_T and figures.get("R", 0) <= GATE_R, figures
    assert figures.get("yaw_drift", 0) <= GATE_YAW_DRIFT and figures.get("t_drift", 0) <= GATE_T_DRIFT and figures.get("r_drift", 0) <= GATE_R, figures


def exceeded(figures, gates):
    """the figures above their gate"""
    return {k: v for k, v in figures.items() if v > gates[k]}


# ------------------------------------------------------------------------------------------------------------------ edge level
def test_edges_against_the_oracle(pg):
    rng = np.random.default_rng(77)
    E = []
    for n in range(200):
        wrap = (0, 1, -1, 0)[n % 4] if n % 5 else 0
        E.append(PO.random_edge(rng, n % 2, wrap=wrap, big_tilt=n % 3 == 0, huber=[None, True, False][n % 3]))
    kind = [e[0] for e in E]
    r, J, c = pg.eval_edges(kind, [e[1][0] for e in E], [e[1][1:] for e in E], [e[2][0] for e in E], [e[2][1:] for e in E], [e[3] for e in E])
    worst = dict(r=0.0, J=0.0, c=0.0)
    wrapped = active = inactive = tilted = 0
    for n, (k, xi, xj, meas) in enumerate(E):
        co, ro, Ji, Jj = PO.edge(k, xi, xj, meas)
        raw = PO.edge(k, xi, xj, meas, correct=False)[1]
        wrapped += abs(xj[0] - xi[0] - meas[3]) > 180.0
        active += k == 1 and raw @ raw > 0.01; inactive += k == 1 and raw @ raw <= 0.01
        tilted += max(abs(meas[4]), abs(meas[5])) > 45.0
        worst["r"] = max(worst["r"], np.abs(r[n] - ro).max()); worst["c"] = max(worst["c"], abs(c[n] - co))
        worst["J"] = max(worst["J"], np.abs(J[n, 0] - Ji).max(), np.abs(J[n, 1] - Jj).max())
    assert wrapped >= 40 and active >= 20 and inactive >= 20 and tilted >= 20, (wrapped, active, inactive, tilted)
    print("measured:", worst)
    assert max(worst.values()) <= GATE_EDGE, worst
    # without the loss (huber_delta <= 0) a loop edge is its plain weighted residual
    r0, _, c0 = pg.eval_edges(kind, [e[1][0] for e in E], [e[1][1:] for e in E], [e[2][0] for e in E], [e[2][1:] for e in E], [e[3] for e in E],
                              pg.default_options(huber_delta=0.0))
    for n, (k, xi, xj, meas) in enumerate(E):
        raw = PO.edge(k, xi, xj, meas, correct=False)[1]
        assert np.abs(r0[n] - raw).max() <= GATE_EDGE * max(1.0, np.abs(raw).max()) and abs(c0[n] - 0.5 * raw @ raw) <= GATE_EDGE * max(1.0, raw @ raw)


# ------------------------------------------------------------------------------------------------------------------ solve level
def test_every_graph_solo_against_the_oracle(pg):
    figures = {}
    for name, ref in reference().items():
        compare(device(pg)["solo"][name], ref, figures)
    gate(figures)


def test_every_graph_in_one_ragged_batch_against_the_oracle(pg):
    figures = {}
    for name, ref in reference().items():
        compare(device(pg)["batch"][name], ref, figures)
    gate(figures)


def same_bits(a, b):
    sa, sb = a["summary"], b["summary"]
    keys = ("cost", "cost_candidate", "rho", "radius", "r_drift", "t_drift")
    return (np.array_equal(a["t"], b["t"]) and np.array_equal(a["R"], b["R"]) and all(np.array_equal(sa[k], sb[k]) for k in keys)
            and all(sa[k] == sb[k] for k in ("iterations", "termination", "initial_cost", "final_cost", "yaw_drift", "step")))


def test_bit_identical_run_to_run_solo_to_batch_and_under_permutation(pg):
    names = list(graphs())
    d = device(pg)
    again = dict(zip(names, pg.optimize([graphs()[k] for k in names])))
    perm = list(np.random.default_rng(5).permutation(len(names)))
    assert perm != sorted(perm)
    shuffled = dict(zip([names[i] for i in perm], pg.optimize([graphs()[names[i]] for i in perm])))
    for k in names:
        assert same_bits(d["batch"][k], again[k]), k
        assert same_bits(d["batch"][k], d["solo"][k]), k
        assert same_bits(d["batch"][k], shuffled[k]), k
    # a batch holding one graph several times: every copy the same
    rep = pg.optimize([graphs()["n300"]] * 3 + [graphs()["n16_shared_newer"]] * 2)
    assert same_bits(rep[0], rep[2]) and same_bits(rep[0], d["solo"]["n300"]) and same_bits(rep[3], rep[4])


def test_trivial_graphs_come_back_unchanged(pg):
    for name in ("n1", "n12_no_loops"):
        g, ref, dev = graphs()[name], reference()[name], device(pg)["solo"][name]
        assert ref["summary"]["termination"] == "CONVERGENCE_GRADIENT" and len(ref["summary"]["iterations"]) == 1
        assert dev["summary"]["termination"] == 1 and dev["summary"]["iterations"] == 1
        assert np.array_equal(dev["t"], np.asarray(g["t"]))
        assert np.abs(dev["R"] - np.array([PO.q2R(q) for q in g["q"]])).max() < 1e-14
        assert abs(dev["summary"]["yaw_drift"]) < 1e-12 and np.abs(dev["summary"]["t_drift"]).max() < 1e-12


# ------------------------------------------------------------------------------------------- termination and step paths
def solve_both(pg, name, opt=None, ceres=None, **dev_opt):
    ref = PO.solve(graphs()[name], opt=opt, ceres=ceres)
    dev = pg.optimize([graphs()[name]], pg.default_options(**dev_opt))[0]
    return ref, dev


def test_function_tolerance_is_the_normal_end(pg):
    n = 0
    for name, ref in reference().items():
        if ref["summary"]["termination"] == "CONVERGENCE_FUNCTION":
            n += 1
            assert 2 <= len(ref["summary"]["iterations"]) - 1 <= 5
            assert device(pg)["solo"][name]["summary"]["termination"] == 3
            assert ref["summary"]["iterations"][-1]["step"] == 0      # the last candidate is not taken
    assert n >= 6


def test_iteration_cap(pg):
    ref, dev = solve_both(pg, "n16_shared_newer", opt=dict(max_num_iterations=1), max_num_iterations=1)
    assert ref["summary"]["termination"] == "NO_CONVERGENCE" and trace_of(ref["summary"]) == (2, [1, 1], 0)
    f = {}
    compare(dev, ref, f); gate(f)
    ref5, dev5 = reference()["n300"], device(pg)["solo"]["n300"]
    assert ref5["summary"]["termination"] == "NO_CONVERGENCE" and len(ref5["summary"]["iterations"]) == 6 and dev5["summary"]["termination"] == 0


def test_parameter_tolerance(pg):
    ref, dev = solve_both(pg, "n12_const_and_free_old", ceres=dict(parameter_tolerance=1.0), parameter_tolerance=1.0)
    assert ref["summary"]["termination"] == "CONVERGENCE_PARAMETER" and trace_of(ref["summary"]) == (2, [1, 0], 2)
    f = {}
    compare(dev, ref, f); gate(f)
    assert np.array_equal(dev["t"], np.asarray(graphs()["n12_const_and_free_old"]["t"]))      # the candidate is not taken


def test_gradient_tolerance(pg):
    ref, dev = reference()["n12_no_loops"], device(pg)["solo"]["n12_no_loops"]
    assert ref["summary"]["termination"] == "CONVERGENCE_GRADIENT" and ref["summary"]["num_free_nodes"] == 11
    assert trace_of(dev["summary"]) == (1, [1], 1)
    # after an accepted step: a tolerance the first step's gradient already meets
    J, r, _ = PO.Graph(graphs()["n2"]).linearize(PO.solve(graphs()["n2"], opt=dict(max_num_iterations=1))["x"])
    g1 = float(np.max(np.abs(J.T @ r)))      # 2.2e-6
    ref, dev = solve_both(pg, "n2", ceres=dict(gradient_tolerance=10 * g1), gradient_tolerance=10 * g1)
    assert ref["summary"]["termination"] == "CONVERGENCE_GRADIENT" and trace_of(ref["summary"]) == (2, [1, 1], 1)
    f = {}
    compare(dev, ref, f); gate(f)


def test_rejected_steps_shrink_the_radius(pg):
    """min_relative_decrease between the first two rho of a case: the first step is accepted, the later ones rejected; the radius
    halves, then quarters (LevenbergMarquardtStrategy::StepRejected)"""
    name = "n16_consecutive_borders"
    rho = [i["rho"] for i in reference()[name]["summary"]["iterations"]]
    assert rho[1] > rho[2] + 1e-3      # 1.1677, 1.1655
    mrd = 0.5 * (rho[1] + rho[2])
    ref, dev = solve_both(pg, name, ceres=dict(min_relative_decrease=mrd), min_relative_decrease=mrd)
    steps = [i["step"] for i in ref["summary"]["iterations"]]
    rad = [i["radius"] for i in ref["summary"]["iterations"]]
    assert steps[:2] == [1, 1] and 0 in steps[2:] and ref["summary"]["termination"] == "NO_CONVERGENCE"
    k = steps.index(0)
    assert steps[k:k + 3] == [0, 0, 0] and rad[k + 1] == rad[k] / 2 and rad[k + 2] == rad[k + 1] / 4
    f = {}
    compare(dev, ref, f); gate(f)
    assert np.array_equal(dev["summary"]["radius"][k:k + 3], np.array(rad[k:k + 3])) or np.allclose(dev["summary"]["radius"][k:k + 3], rad[k:k + 3], rtol=1e-9)
    assert dev["summary"]["radius"][k + 1] == dev["summary"]["radius"][k] / 2 and dev["summary"]["radius"][k + 2] == dev["summary"]["radius"][k + 1] / 4


def test_options_reach_the_kernel(pg):
    """no loss, another weight and yaw divisor: device and oracle move together"""
    kw = dict(huber_delta=0.0, loop_weight=2.0, loop_yaw_divisor=4.0)
    ref, dev = solve_both(pg, "n12_huber", opt=kw, **kw)
    assert ref["summary"]["final_cost"] > 10 * reference()["n12_huber"]["summary"]["final_cost"]      # the gross loop edge is no longer tamed
    f = {}
    compare(dev, ref, f); gate(f)


# ------------------------------------------------------------------------------- panel, chunk, tile and thread-count boundaries
@functools.lru_cache(maxsize=None)
def boundary():
    """(graphs, oracle results) of pose_graph_oracle.boundary_graphs(): made once, shared, never changed"""
    G = PO.boundary_graphs()
    return G, {k: PO.solve(g) for k, g in G.items()}


def test_boundary_shapes_solo_and_in_one_ragged_batch(pg):
    """every size built into the kernel (band chunk 20, W chunk 32, panel 301 / 320, Schur tile 64, 256 threads, 256 loops) with a graph on
    it and one next to it; tests/test_pose_graph_cpu.py holds every one of them to its shape and to decisions 1 % clear of their thresholds"""
    G, ref = boundary()
    names = list(G)
    solo = {k: pg.optimize([G[k]])[0] for k in names}
    batch = dict(zip(names, pg.optimize([G[k] for k in names])))
    back = dict(zip(names[::-1], pg.optimize([G[k] for k in names[::-1]])))
    worst = {}
    print()
    for k in names:
        f = {}
        compare(solo[k], ref[k], f)
        compare(batch[k], ref[k], f)
        compare(back[k], ref[k], f)
        print("%-10s recs %d term %d  " % (k, solo[k]["summary"]["iterations"], solo[k]["summary"]["termination"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for key, v in f.items():
            worst[key] = max(worst.get(key, 0.0), v)
        assert same_bits(solo[k], batch[k]), k
        assert same_bits(solo[k], back[k]), k
    print("measured:", {k: "%.3g" % v for k, v in worst.items()})
    assert not exceeded(worst, BOUNDARY_GATES), exceeded(worst, BOUNDARY_GATES)


def test_trace_longer_than_the_record_cap(pg):
    """more records than TCV_POSE_GRAPH_MAX_TRACE: `iterations` counts them all, the first 16 are kept, nothing is written past them"""
    kw = dict(max_num_iterations=20, initial_trust_region_radius=1e-8, function_tolerance=0.0, parameter_tolerance=0.0)
    ceres = {k: v for k, v in kw.items() if k != "max_num_iterations"}
    opts = pg.default_options(**kw)
    long_names = ("n16_shared_newer", "n20_sequences")
    solo = {}
    for name in long_names:
        ref = PO.solve(graphs()[name], opt=dict(max_num_iterations=20), ceres=ceres)
        so, its = ref["summary"], ref["summary"]["iterations"]
        assert trace_of(so) == (21, [1] * 21, 0) and len(its) > pg.MAX_TRACE
        assert all(abs(i["rho"] - 1.0) < 0.08 for i in its[1:])
        assert all(b["radius"] == a["radius"] / (1.0 / 3.0) for a, b in zip(its[1:], its[2:])) and its[1]["radius"] == 1e-8      # StepAccepted at its clamp: tripled
        dev = solo[name] = pg.optimize([graphs()[name]], opts)[0]
        s = dev["summary"]
        assert s["iterations"] == 21 and s["termination"] == 0
        T = pg.MAX_TRACE
        assert s["step"] == [1] * T and all(len(s[k]) == T for k in ("cost", "cost_candidate", "rho", "radius"))
        assert np.array_equal(s["radius"], [i["radius"] for i in its[:T]])
        worst_rho = 0.0
        for n, rec in enumerate(its[:T]):
            for key in ("cost", "cost_candidate"):
                assert abs(s[key][n] - rec[key]) <= GATE_COST_REL * abs(rec[key]), (name, n, key)
            if n:
                # rho = (cost - candidate) / model_cost_change: two costs, each within GATE_COST_REL of the oracle's, over a model change that is
                # 1e-9 .. 1e-2 of them; the second term is three times what well-scaled records measure (the header of this file)
                bound = 2.0 * GATE_COST_REL * its[n - 1]["cost"] / abs(rec["model_cost_change"]) + 3 * 1.5e-11
                print("%s record %2d  cost %.3e  model change %.3e  rho off by %.2e  bound %.2e" % (name, n, rec["cost"], rec["model_cost_change"], abs(s["rho"][n] - rec["rho"]), bound))
                assert abs(s["rho"][n] - rec["rho"]) <= bound, (name, n, s["rho"][n], rec["rho"], bound)
                worst_rho = max(worst_rho, abs(s["rho"][n] - rec["rho"]))
        f = dict(cost_rel=abs(s["final_cost"] - so["final_cost"]) / so["final_cost"], t=np.abs(dev["t"] - ref["t"]).max(), R=np.abs(dev["R"] - ref["R"]).max(),
                 yaw_drift=abs(s["yaw_drift"] - so["yaw_drift"]), t_drift=np.abs(s["t_drift"] - so["t_drift"]).max(), r_drift=np.abs(s["r_drift"] - so["r_drift"]).max())
        assert abs(s["initial_cost"] - so["initial_cost"]) <= GATE_COST_REL * so["initial_cost"]
        print(name, "worst rho", "%.2e" % worst_rho)
        gate(f)
    # in a batch: the record of a long trace ends where the next graph's poses begin.  The only traces that stay short under these
    # options are those that end at entry, so the two long graphs also sit next to each other
    short = {k: pg.optimize([graphs()[k]], opts)[0] for k in ("n12_no_loops", "n1")}
    assert all(v["summary"]["iterations"] == 1 for v in short.values())
    order = ["n12_no_loops", "n16_shared_newer", "n20_sequences", "n1"]
    for k, dev in zip(order, pg.optimize([graphs()[k] for k in order], opts)):
        assert same_bits(dev, solo[k] if k in solo else short[k]), k


# ------------------------------------------------------------------------------------------------------------ limits, drift
def test_limits_launch_nothing(pg):
    import tcv
    n = pg.MAX_NODES + 1
    big = pg.Graph(dict(t=np.zeros((n, 3)), q=np.tile([0.0, 0, 0, 1], (n, 1)), loops=[]))
    ok = pg.Graph(graphs()["n5"])
    live0 = tcv.device_memory_stats()[0]
    rc, t_out, _, sums = pg.optimize_raw([ok.desc, big.desc])
    assert rc == tcv.TCV_ERR_UNSUPPORTED and not t_out[0].any() and sums[0].iterations == 0      # nothing ran, nothing was written
    assert tcv.device_memory_stats()[0] == live0


def test_drift_reproduces_the_last_node(pg):
    for name, dev in device(pg)["batch"].items():
        g, s, so = graphs()[name], dev["summary"], reference()[name]["summary"]
        assert abs(s["yaw_drift"] - so["yaw_drift"]) <= GATE_YAW_DRIFT and np.abs(s["t_drift"] - so["t_drift"]).max() <= GATE_T_DRIFT
        assert np.abs(s["r_drift"] - so["r_drift"]).max() <= GATE_R
        t_vio = np.asarray(g["t"])[-1]
        assert np.abs(s["r_drift"] @ t_vio + s["t_drift"] - dev["t"][-1]).max() < 1e-12 * max(1.0, np.abs(t_vio).max())
        assert np.abs(s["r_drift"] - PO.ypr2R(s["yaw_drift"], 0, 0)).max() < 1e-14
    assert abs(device(pg)["batch"]["n300"]["summary"]["yaw_drift"]) > 0.1      # a drift worth correcting
