"""Batched bundle adjustment of the initial SfM on the device (include/tcv_sfm_ba.h, csrc/tcv_sfm_ba.hip) against its NumPy restatement
(tests/sfm_ba_oracle.py): the observation maths on seeded observations, every problem of sfm_ba_oracle.test_problems() solved once alone and
once in one ragged batch, the shapes at which the kernel can go wrong, every termination and step path (asserted on the ORACLE's trace first,
so that no test passes vacuously), bit-exact determinism, the world-frame pair and a structure fuzzer.  Every problem whose trace is
compared has an oracle decision margin of at least 1e-6 (asserted).

Gates.  Traces (records, accepted / rejected per record, termination code, `accepted`) must be identical.  Every numerical gate is three
times the worst figure measured on an MI355X over the tests of this file that use it (profiles/sfm_ba.txt has the table per problem); none
on a state is looser than the project's 1e-6 criterion:
    observation residual / Jacobian / cost, absolute    measured 1.1e-15 / 6.8e-16 / 3.0e-17      gate 3.3e-15 (three times the largest)
    costs of the trace, relative (costs >= 1e-12)       measured 1.05e-11 (one_point_six_frames)  gate 3.2e-11
    rho of the trace, over max(1, |rho|)                measured 1.01e-6  (f3_l1, ending record)  gate 3.1e-6
    rho of every record but the ending one              measured 4.8e-9   (f3_l1)                 gate 1.5e-8
    quaternion entries, absolute                        measured 1.6e-13  (one_point_six_frames)  gate 4.8e-13
    translations / points, over max(1, largest entry)   measured 1.6e-12 / 9.1e-14                gate 4.8e-12 / 2.8e-13
Costs below 1e-12 (exact data, a single point that every frame fits) are rounding of the residuals: their difference must stay inside
1e-15 sqrt(2 cost n_residuals), a reasoned bound (compare()); the largest share of it measured is 1.6 %.  rho of the record that ends a
solve on the function tolerance divides a cost change of <= 1e-6 of the cost by a model change of the same size: the 1e-14 relative
rounding of the two costs arrives there multiplied by 1e6 and more.  States are compared relative to the largest entry of their family
(at least 1): the 1e-6 criterion is relative.
The boundary sweep (sfm_ba_oracle.boundary_problems()) stays inside these gates (worst: costs 9.4e-12, rho 5.7e-7 / 2.8e-9, states 6.7e-13).
Two named problems have gates of their own, three times their own worst, because their linear systems are ill-conditioned (HARD):
    no_convergence   costs 4.1e-7, rho 4.1e-7, quaternions 1.3e-10, translations 4.5e-9, points 6.8e-9   gates 1.3e-6, 1.3e-6, 4.1e-10, 1.4e-8, 2.1e-8
        pose noise 0.3, point noise 1.5: the trace never converges and throws points out to 1.2e4 m and a camera to 2.8e3 m; the oracle's
        damped normal matrix has cond x eps from 8e-3 (radius 1.5) to above 1 (radius 5e3) along the trace, so a step carries two digits in
        its worst directions and fifty of them follow each other.  The trace is still identical and every state agrees to 7e-9 of its size.
    rejected         costs 1.0e-8, rho 1.0e-8 (the same record), states 1.7e-14: inside the gates above
        its first rejected candidate costs 2.7e5 times the model's change (rho -2.7e5): the cost there rises steeply along the step, and
        the step's relative error (cond x eps 1e-10) arrives multiplied by that slope.
The structure fuzzer (tests/dev/fuzz_sfm_ba.py, seeds 0 .. 29) uses the gates above where its worst stays inside them and three times its
own worst elsewhere:
    costs 4.3e-10 (seed 8)   gate 1.3e-9      a 37-record trace whose last costs fall from 2e-10 to the 1e-12 line of the relative figure
    rho before the end 1.8e-8 (seed 15)  gate 5.6e-8
    translations 2.6e-10 (seed 17), points 9.2e-9 (seed 18)   gates 7.8e-10, 2.8e-8
        seed 17: 7 points for 15 frames, the radius grows to 1.7e10 and leaves cond x eps = 1.6e-4 to the damping alone; seed 18: 33 points
        seen by two frames each, 51 records without convergence, points out to 2.6e3 m, cond x eps from 9e-5 to above 1.
The non-finite-candidate rule (a candidate whose residuals are not finite costs DBL_MAX and is rejected) is built and untested: no seed of
the generator reached it on the CPU (profiles/sfm_ba.txt)."""
import functools
import os
import sys

import numpy as np
import pytest

import sfm_ba_oracle as BO

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-6
GATE_OBS = 3.3e-15
COST_FLOOR = 1e-15
TINY_COST = 1e-12
FILE_GATES = dict(cost_rel=3.2e-11, rho=3.1e-6, rho_before_end=1.5e-8, q=4.8e-13, t=4.8e-12, X=2.8e-13)
HARD = ("rejected", "no_convergence")      # the two problems with gates of their own (the docstring says why)
HARD_GATES = dict(cost_rel=1.3e-6, rho=1.3e-6, rho_before_end=1.3e-6, q=4.1e-10, t=1.4e-8, X=2.1e-8)
BOUNDARY_GATES = dict(FILE_GATES)
FUZZ_GATES = dict(FILE_GATES, cost_rel=1.3e-9, rho_before_end=5.6e-8, t=7.8e-10, X=2.8e-8)


@pytest.fixture(scope="module")
def ba(gpu):
    import tcv_sfm_ba
    return tcv_sfm_ba


@functools.lru_cache(maxsize=None)
def problems():
    return BO.test_problems()


@functools.lru_cache(maxsize=None)
def reference():
    """the oracle's answer for every test problem at the reference's options: made once, shared, never changed"""
    return {k: BO.solve(p) for k, p in problems().items()}


_device = {}


def device(ba):
    """every problem solved alone, and all of them in one batch: made once"""
    if not _device:
        names = list(problems())
        _device["solo"] = {k: ba.bundle_adjust([problems()[k]])[0] for k in names}
        _device["batch"] = dict(zip(names, ba.bundle_adjust([problems()[k] for k in names])))
    return _device


def trace_of(summary):
    """(number of records, step per record, termination code, accepted) of an oracle or a device summary"""
    if isinstance(summary["iterations"], int):
        return summary["iterations"], list(summary["step"]), summary["termination"], bool(summary["accepted"])
    return len(summary["iterations"]), [i["step"] for i in summary["iterations"]], summary["termination_code"], bool(summary["accepted"])


def compare(dev, ref, figures, problem=None, ceres=None):
    """traces identical (the oracle's decisions at least MIN_MARGIN clear of their thresholds; ceres: the overrides the oracle solved
    with); the numerical differences go into `figures`"""
    s, so = dev["summary"], ref["summary"]
    assert BO.decision_margin(so, ceres)[0] >= MIN_MARGIN, BO.decision_margin(so, ceres)
    n = len(so["iterations"])
    T = min(n, len(s["cost"]))
    assert trace_of(s)[0] == n and trace_of(s)[1] == trace_of(so)[1][:T] and trace_of(s)[2:] == trace_of(so)[2:], (trace_of(s), trace_of(so))
    assert (s["num_camera_unknowns"], s["num_points"], s["num_observations"]) == (so["num_camera_unknowns"], so["num_points"], so["num_observations"])
    for k in ("c_rotation", "c_translation", "position", "q", "T"):
        assert np.all(np.isfinite(dev[k])), k

    def upd(k, v):
        figures[k] = max(figures.get(k, 0.0), float(v))

    # a cost is half a sum of n_res squares of residuals that each carry a few ulps of a normalised image coordinate (of order 1, so about
    # 1e-15): its error is at least 1e-15 sqrt(2 cost n_res), which is all that is left of a cost at rounding level (exact data, a single
    # point that every frame fits).  Costs of TINY_COST and more go into the relative figure; below it the difference must stay inside
    # that bound, which is reasoned, not measured (the largest share of it seen on an MI355X: 1.6 %, `exact`).
    n_res = 2 * so["num_observations"]

    def cost_figure(a, b):
        a, b = np.asarray(a, float), np.asarray(b, float)
        big = (np.abs(a) >= TINY_COST) & (np.abs(a) < 1e300)
        small = np.abs(a) < TINY_COST
        assert np.all(np.abs(a - b)[small] <= COST_FLOOR * np.sqrt(2.0 * np.abs(a[small]) * n_res) + 1e-300), (a[small], b[small])
        return float(np.max(np.abs(a - b)[big] / np.abs(a[big]))) if big.any() else 0.0

    its = so["iterations"][:T]
    for key in ("cost", "cost_candidate"):
        if T:
            upd("cost_rel", cost_figure([i[key] for i in its], s[key][:T]))
    if its:
        upd("cost_rel", cost_figure([so["initial_cost"], so["final_cost"]], [s["initial_cost"], s["final_cost"]]))
        # rho relative to max(1, |rho|): a rejected step's candidate may cost 1e5 times the model's change
        rho_o = np.array([i["rho"] for i in its])
        d_rho = np.abs(rho_o - s["rho"][:T]) / np.maximum(1.0, np.abs(rho_o))
        upd("rho", np.max(d_rho))
        ends_on_a_tolerance = so["termination"] in ("CONVERGENCE_FUNCTION", "CONVERGENCE_PARAMETER") and T == n      # (that record's rho divides a vanishing cost change)
        upd("rho_before_end", (np.max(d_rho[:T - 1]) if T > 1 else 0.0) if ends_on_a_tolerance else np.max(d_rho))
        assert np.allclose([i["radius"] for i in its], s["radius"][:T], rtol=1e-6, atol=0)      # a function of the accepted steps' rho, cubed
    # states relative to the largest entry of their family, at least 1 (quaternion entries are at most 1: absolute)
    for key, fam in (("q", "c_rotation"), ("t", "c_translation"), ("X", "position")):
        upd(key, np.max(np.abs(dev[fam] - ref[fam])) / max(1.0, np.max(np.abs(ref[fam]))))
    # the constants of :248-255 come back as given
    if problem is not None:
        l, F = int(problem["l"]), len(dev["c_rotation"])
        assert np.array_equal(dev["c_rotation"][l], np.asarray(problem["c_rotation"])[l]) and np.array_equal(dev["c_translation"][l], np.asarray(problem["c_translation"])[l])
        assert np.array_equal(dev["c_translation"][F - 1], np.asarray(problem["c_translation"])[F - 1])


def exceeded(figures, gates):
    """the figures above their gate"""
    return {k: v for k, v in figures.items() if v > gates[k]}


def gate(figures, gates=None, quiet=False):
    if not quiet:
        print("measured:", {k: "%.3g" % v for k, v in figures.items()})
    bad = exceeded(figures, gates or FILE_GATES)
    assert not bad, bad


def same_bits(a, b):
    sa, sb = a["summary"], b["summary"]
    keys = ("cost", "cost_candidate", "rho", "radius")
    return (all(np.array_equal(a[k], b[k]) for k in ("c_rotation", "c_translation", "position", "q", "T")) and all(np.array_equal(sa[k], sb[k]) for k in keys)
            and all(sa[k] == sb[k] for k in ("iterations", "termination", "accepted", "initial_cost", "final_cost", "step")))


# ------------------------------------------------------------------------------------------------------------ observation level
def test_observations_against_the_oracle(ba):
    rng = np.random.default_rng(77)
    q, t, X, uv = BO.random_observations(rng, 240)
    norms = np.linalg.norm(q, axis=1)
    assert (q[:, 0] < 0).sum() >= 50 and (np.abs(norms - 1) > 9e-4).sum() >= 70 and (np.abs(norms - 1) < 1e-12).sum() >= 100
    ro, Jo, co = BO.observations(q, t, X, uv)
    assert (np.abs(ro[:, 0] + uv[:, 0]) > 0.9).sum() >= 40      # points next to the image plane's edge (|u| about 1)
    r, J, c = ba.eval_observations(q, t, X, uv)
    worst = dict(r=np.abs(r - ro).max(), J=np.abs(J - Jo).max() / max(1.0, np.abs(Jo).max()), c=np.abs(c - co).max())
    print("measured:", worst, "largest |J|", np.abs(Jo).max())
    assert max(worst.values()) <= GATE_OBS, worst
    # the norm of the quaternion cancels: the same observation at twice the norm
    r2, J2, c2 = ba.eval_observations(2.0 * q, t, X, uv)
    assert np.abs(r2 - r).max() <= GATE_OBS and np.abs(J2 - J).max() <= GATE_OBS * max(1.0, np.abs(Jo).max())


# ------------------------------------------------------------------------------------------------------------------ solve level
def against_the_oracle(ba, which):
    figures, hard = {}, {}
    print()
    for name, ref in reference().items():
        f = {}
        compare(device(ba)[which][name], ref, f, problems()[name])
        print("%-22s recs %2d term %d  " % (name, len(ref["summary"]["iterations"]), ref["summary"]["termination_code"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        into = hard if name in HARD else figures
        for k, v in f.items():
            into[k] = max(into.get(k, 0.0), v)
    gate(figures)
    gate(hard, HARD_GATES)


def test_every_problem_solo_against_the_oracle(ba):
    against_the_oracle(ba, "solo")


def test_every_problem_in_one_ragged_batch_against_the_oracle(ba):
    against_the_oracle(ba, "batch")


def test_bit_identical_run_to_run_solo_to_batch_and_under_permutation(ba):
    names = list(problems())
    d = device(ba)
    again = dict(zip(names, ba.bundle_adjust([problems()[k] for k in names])))
    perm = list(np.random.default_rng(5).permutation(len(names)))
    assert perm != sorted(perm)
    shuffled = dict(zip([names[i] for i in perm], ba.bundle_adjust([problems()[names[i]] for i in perm])))
    for k in names:
        assert same_bits(d["batch"][k], again[k]), k
        assert same_bits(d["batch"][k], d["solo"][k]), k
        assert same_bits(d["batch"][k], shuffled[k]), k
    rep = ba.bundle_adjust([problems()["f11_l9_p150"]] * 3 + [problems()["f2_l0"]] * 2)
    assert same_bits(rep[0], rep[2]) and same_bits(rep[0], d["solo"]["f11_l9_p150"]) and same_bits(rep[3], rep[4])


def test_world_frame_pair_is_the_reference_lines_on_the_camera_frame_outputs(ba):
    for name, dev in device(ba)["batch"].items():
        q, T = BO.world_frame(dev["c_rotation"], dev["c_translation"])      # :290-303 as a NumPy line on the DEVICE's camera-frame outputs
        assert np.array_equal(dev["q"], q) and np.array_equal(dev["T"], T), name
        # and it is what the reference means: a camera centre
        R = BO.quat_matrix(dev["c_rotation"])
        assert np.abs(T + np.einsum("nji,nj->ni", R, dev["c_translation"])).max() < 1e-12
    # optional: without the two arrays the call does not write them
    p = ba.Problem(problems()["f3_l1"])
    rc, out, res = ba.bundle_adjust_raw([p.desc], world_frame=False)
    assert rc == 0 and not out[0]["q"].any() and not out[0]["T"].any() and np.array_equal(out[0]["position"], device(ba)["solo"]["f3_l1"]["position"])


# --------------------------------------------------------------------------------------------------------------------- shapes
def test_shapes_of_the_named_problems(ba):
    d, P = device(ba)["solo"], problems()
    assert d["f2_l0"]["summary"]["num_camera_unknowns"] == 3 and d["f3_l1"]["summary"]["num_camera_unknowns"] == 9
    for k in ("f11_l0_p40", "f11_l5_p90", "f11_l9_p150"):
        assert d[k]["summary"]["num_camera_unknowns"] == 57
    assert [P[k]["l"] for k in ("f11_l0_p40", "f11_l5_p90", "f11_l9_p150")] == [0, 5, 9]
    assert d["one_point_six_frames"]["summary"]["num_points"] == 1
    counts = [len(o) for o in P["two_and_all"]["observations"]]
    assert counts[0] == 2 and counts[1] == 11
    # a free frame that no point observes must not move: not a bit
    assert not any(o[0] == 4 for po in P["idle_frame"]["observations"] for o in po)
    for dev in (d["idle_frame"], device(ba)["batch"]["idle_frame"]):
        assert np.array_equal(dev["c_rotation"][4], P["idle_frame"]["c_rotation"][4]) and np.array_equal(dev["c_translation"][4], P["idle_frame"]["c_translation"][4])
        assert np.abs(dev["c_rotation"][3] - P["idle_frame"]["c_rotation"][3]).max() > 1e-4      # its neighbours do
    # points seen only by the frames whose translation is constant (l and F - 1): they move, by the rotation of F - 1 and themselves
    assert all([o[0] for o in po] == [2, 10] for po in P["constant_frames_only"]["observations"][:6])
    assert np.abs(d["constant_frames_only"]["position"][:6] - P["constant_frames_only"]["position"][:6]).max() > 1e-3


@functools.lru_cache(maxsize=None)
def boundary():
    """(problems, oracle results) of sfm_ba_oracle.boundary_problems(): made once, shared, never changed"""
    G = BO.boundary_problems()
    return G, {k: BO.solve(p) for k, p in G.items()}


def test_boundary_shapes_solo_and_in_one_ragged_batch(ba):
    """every size built into the kernel (16 points per Schur chunk, 256 point owners, tiles of 4 over nc + 1 rows, the point and frame limits)
    with a problem on it and one next to it"""
    G, ref = boundary()
    names = list(G)
    solo = {k: ba.bundle_adjust([G[k]])[0] for k in names}
    batch = dict(zip(names, ba.bundle_adjust([G[k] for k in names])))
    back = dict(zip(names[::-1], ba.bundle_adjust([G[k] for k in names[::-1]])))
    worst = {}
    print()
    for k in names:
        f = {}
        compare(solo[k], ref[k], f, G[k])
        compare(batch[k], ref[k], f, G[k])
        compare(back[k], ref[k], f, G[k])
        print("%-14s recs %d term %d  " % (k, solo[k]["summary"]["iterations"], solo[k]["summary"]["termination"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for key, v in f.items():
            worst[key] = max(worst.get(key, 0.0), v)
        assert same_bits(solo[k], batch[k]), k
        assert same_bits(solo[k], back[k]), k
    gate(worst, BOUNDARY_GATES)


# ------------------------------------------------------------------------------------------- termination and step paths
def solve_both(ba, name, ceres=None, problem=None, **dev_opt):
    p = problem if problem is not None else problems()[name]
    ref = BO.solve(p, ceres=ceres)
    dev = ba.bundle_adjust([p], ba.default_options(**dev_opt))[0]
    return ref, dev


def test_function_tolerance_is_the_normal_end(ba):
    n = 0
    for name, ref in reference().items():
        if ref["summary"]["termination"] == "CONVERGENCE_FUNCTION":
            n += 1
            assert device(ba)["solo"][name]["summary"]["termination"] == 3 and device(ba)["solo"][name]["summary"]["accepted"]
            assert ref["summary"]["iterations"][-1]["step"] == 0      # the last candidate is not taken
    assert n >= 8
    for k in ("f11_l0_p40", "f11_l5_p90", "f11_l9_p150"):
        assert 5 <= len(reference()[k]["summary"]["iterations"]) <= 8


def test_gradient_tolerance_at_entry_and_after_accepted_steps(ba):
    ref, dev = reference()["exact"], device(ba)["solo"]["exact"]
    assert ref["summary"]["termination"] == "CONVERGENCE_GRADIENT" and len(ref["summary"]["iterations"]) == 1
    assert trace_of(dev["summary"]) == (1, [1], 1, True)
    for k in ("c_rotation", "c_translation", "position"):
        assert np.array_equal(dev[k], np.asarray(problems()["exact"][k]))      # nothing moved
    ref, dev = reference()["one_point_six_frames"], device(ba)["solo"]["one_point_six_frames"]
    assert ref["summary"]["termination"] == "CONVERGENCE_GRADIENT" and trace_of(ref["summary"])[:3] == (4, [1, 1, 1, 1], 1)
    assert trace_of(dev["summary"]) == (4, [1, 1, 1, 1], 1, True)


def test_parameter_tolerance(ba):
    """parameter_tolerance raised until the oracle ends on it"""
    ref, dev = solve_both(ba, "f11_l0_p40", ceres=dict(parameter_tolerance=1e-3), parameter_tolerance=1e-3)
    so = ref["summary"]
    assert so["termination"] == "CONVERGENCE_PARAMETER" and so["iterations"][-1]["step"] == 0 and len(so["iterations"]) >= 3
    f = {}
    compare(dev, ref, f, problems()["f11_l0_p40"], ceres=dict(parameter_tolerance=1e-3)); gate(f)


def test_rejected_steps_shrink_the_radius(ba):
    ref, dev = reference()["rejected"], device(ba)["solo"]["rejected"]
    steps = [i["step"] for i in ref["summary"]["iterations"]]
    rad = [i["radius"] for i in ref["summary"]["iterations"]]
    k = steps.index(0)
    assert 0 < k < len(steps) - 2 and steps[k:k + 2] == [0, 0] and rad[k + 1] == rad[k] / 2 and ref["summary"]["termination"] == "CONVERGENCE_FUNCTION"
    s = dev["summary"]
    assert s["step"] == steps and s["radius"][k + 1] == s["radius"][k] / 2 and s["radius"][k + 2] == s["radius"][k + 1] / 4


def test_iteration_cap_at_three_is_accepted_on_its_cost(ba):
    ref, dev = solve_both(ba, "f2_l0", ceres=dict(max_num_iterations=3), max_num_iterations=3)
    so = ref["summary"]
    assert so["termination"] == "NO_CONVERGENCE" and trace_of(so) == (4, [1, 1, 1, 1], 0, True) and so["final_cost"] < 5e-3
    f = {}
    compare(dev, ref, f, problems()["f2_l0"]); gate(f)


def test_iteration_cap_at_fifty_is_not_accepted(ba):
    ref, dev = reference()["no_convergence"], device(ba)["solo"]["no_convergence"]
    so = ref["summary"]
    assert so["termination"] == "NO_CONVERGENCE" and len(so["iterations"]) == 51 and so["final_cost"] > 1.0 and not so["accepted"]
    s = dev["summary"]
    assert s["iterations"] == 51 and s["termination"] == 0 and not s["accepted"] and len(s["cost"]) == 51 <= ba.MAX_TRACE


def test_failure_at_entry_leaves_the_state_and_the_neighbours_alone(ba):
    """a point exactly on a camera's plane z = 0: the first residual is not finite"""
    bad = BO.with_point_on_camera_plane(problems()["f3_l1"], 4)
    ref = BO.solve(bad)
    assert ref["summary"]["termination"] == "FAILURE" and ref["summary"]["iterations"] == []
    order = ["f11_l0_p40", None, "f2_l0"]
    res = ba.bundle_adjust([bad if k is None else problems()[k] for k in order])
    s = res[1]["summary"]
    assert (s["iterations"], s["termination"], s["accepted"]) == (0, 5, False) and s["final_cost"] == BO.DBL_MAX == s["initial_cost"]
    for k in ("c_rotation", "c_translation", "position"):
        assert np.array_equal(res[1][k], np.asarray(bad[k])), k      # as given, never NaN
    assert np.all(np.isfinite(res[1]["q"])) and np.all(np.isfinite(res[1]["T"]))
    assert same_bits(res[0], device(ba)["solo"]["f11_l0_p40"]) and same_bits(res[2], device(ba)["solo"]["f2_l0"])


def test_limits_launch_nothing(ba):
    import tcv
    n = ba.MAX_POINTS + 1
    big = ba.Problem(dict(c_rotation=np.tile([1.0, 0, 0, 0], (3, 1)), c_translation=np.zeros((3, 3)), l=0, position=np.tile([0.0, 0, 5.0], (n, 1)),
                          observations=[[(0, 0.0, 0.0), (1, 0.0, 0.0)]] * n))
    ok = ba.Problem(problems()["f3_l1"])
    live0 = tcv.device_memory_stats()[0]
    rc, out, res = ba.bundle_adjust_raw([ok.desc, big.desc])
    assert rc == tcv.TCV_ERR_UNSUPPORTED and not out[0]["position"].any() and res[0].summary.iterations == 0      # nothing ran, nothing was written
    assert tcv.device_memory_stats()[0] == live0


def test_timing_is_reported(ba):
    ba.bundle_adjust([problems()["f11_l9_p150"]])
    t = ba.last_timing()
    assert t["kernel_ms"] > 0.0 and t["upload_ms"] >= 0.0 and t["download_ms"] >= 0.0 and t["pack_ms"] > 0.0


# ------------------------------------------------------------------------------------------------------------------- fuzzer
def test_structure_fuzzer(ba):
    """tests/dev/fuzz_sfm_ba.py, seeds 0 .. 29: random F, l, point counts and visibility, solo and in one ragged batch"""
    dev = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev")
    sys.path.insert(0, dev)
    try:
        import fuzz_sfm_ba as F
    finally:
        sys.path.remove(dev)
    print()
    worst, tally = F.run(ba, compare, same_bits, 30, 0)
    print("terminations:", tally)
    assert tally.get("CONVERGENCE_FUNCTION", 0) >= 10 and tally.get("CONVERGENCE_GRADIENT", 0) >= 3 and tally.get("NO_CONVERGENCE", 0) >= 1, tally
    gate(worst, FUZZ_GATES)
