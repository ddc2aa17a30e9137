"""CPU side of the batched bundle adjustment of the initial SfM (include/tcv_sfm_ba.h): the NumPy restatement (tests/sfm_ba_oracle.py)
against central differences and against scipy's least squares on the same cost, the paths its named test problems are meant to reach, the
input validation of the C-ABI (which runs before the device is touched), the limits, the loud failure without a device, the header as
C99 / C++14, and the host-side plan."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import sfm_ba_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tcv_sfm_ba.h")
MARGIN = 1e-3      # the seeds of the named problems: every decision of the oracle at least this far (relative) from its threshold; the GPU file asks 1e-6


@pytest.fixture(scope="module")
def ba(built):
    import tcv_sfm_ba
    return tcv_sfm_ba


@functools.lru_cache(maxsize=None)
def solved():
    return {k: BO.solve(p) for k, p in BO.test_problems().items()}


def steps_of(summary):
    return [i["step"] for i in summary["iterations"]]


def test_oracle_jacobian_against_central_differences():
    rng = np.random.default_rng(1)
    q, t, X, uv = BO.random_observations(rng, 60)
    assert (q[:, 0] < 0).sum() >= 10 and np.abs(np.linalg.norm(q, axis=1) - 1).max() > 5e-4
    _, J, _ = BO.observations(q, t, X, uv)
    worst, h = 0.0, 1e-6
    for n in range(len(q)):
        def r_at(d):
            return BO.observations(BO.quat_plus(q[n], d[:3])[None], (t[n] + d[3:6])[None], (X[n] + d[6:])[None], uv[n:n + 1], False)[0][0]
        for k in range(9):
            d = np.zeros(9); d[k] = h
            worst = max(worst, float(np.abs((r_at(d) - r_at(-d)) / (2 * h) - J[n, :, k]).max()))
    print("worst difference", worst)
    assert worst < 1e-7, worst      # central differences at h = 1e-6 on values of order 1: truncation + rounding about 1e-9


def test_oracle_final_cost_against_scipy_least_squares():
    so = pytest.importorskip("scipy.optimize")
    for name in ("f3_l1", "f11_l0_p40"):
        p = BO.test_problems()[name]
        ref = BO.solve(p)
        G = BO.Problem(p)
        x0 = G.x0()

        def residuals(v):
            return G.evaluate(G.plus(x0, v), False)[0].ravel()

        res = so.least_squares(residuals, np.zeros(G.nu), xtol=1e-15, ftol=1e-15, gtol=1e-15)
        # the oracle stops on the function tolerance 1e-6: its cost may sit a few 1e-6 (relative) above the minimum, not below its own start
        assert ref["summary"]["final_cost"] <= res.cost * (1 + 1e-4), (name, ref["summary"]["final_cost"], res.cost)
        assert ref["summary"]["final_cost"] >= res.cost * (1 - 1e-9), (name, ref["summary"]["final_cost"], res.cost)


def test_oracle_reaches_every_path_the_gpu_tests_rely_on():
    S = {k: v["summary"] for k, v in solved().items()}
    for k, s in S.items():
        m = BO.decision_margin(s)
        print("%-22s nc %2d obs %4d records %2d %-22s accepted %d margin %.2e (%s, record %d)" % (
            k, s["num_camera_unknowns"], s["num_observations"], len(s["iterations"]), s["termination"], s["accepted"], m[0], m[1], m[2]))
        assert m[0] >= MARGIN, (k, m)
        assert all(i.get("candidate_finite", True) for i in s["iterations"])
    for k in ("f11_l0_p40", "f11_l5_p90", "f11_l9_p150", "f2_l0", "f3_l1"):
        assert S[k]["termination"] == "CONVERGENCE_FUNCTION" and S[k]["accepted"], k
    assert S["exact"]["termination"] == "CONVERGENCE_GRADIENT" and len(S["exact"]["iterations"]) == 1
    assert S["one_point_six_frames"]["termination"] == "CONVERGENCE_GRADIENT" and steps_of(S["one_point_six_frames"]) == [1, 1, 1, 1]
    st = steps_of(S["rejected"])
    assert S["rejected"]["termination"] == "CONVERGENCE_FUNCTION" and 0 in st[1:-1] and st[-2] == 1      # rejected steps in the middle of a converging trace
    s = S["no_convergence"]
    assert s["termination"] == "NO_CONVERGENCE" and len(s["iterations"]) == 51 and s["final_cost"] > 1.0 and not s["accepted"]
    assert S["f2_l0"]["num_camera_unknowns"] == 3 and S["f3_l1"]["num_camera_unknowns"] == 9 and S["f11_l9_p150"]["num_camera_unknowns"] == 57
    # the structures
    P = BO.test_problems()
    counts = [len(o) for o in P["two_and_all"]["observations"]]
    assert counts[0] == 2 and counts[1] == 11
    assert not any(o[0] == 4 for po in P["idle_frame"]["observations"] for o in po)
    assert all([o[0] for o in po] == [2, 10] for po in P["constant_frames_only"]["observations"][:6])
    # a free frame that no point observes does not move
    r = solved()["idle_frame"]
    assert np.array_equal(r["c_rotation"][4], P["idle_frame"]["c_rotation"][4]) and np.array_equal(r["c_translation"][4], P["idle_frame"]["c_translation"][4])
    assert np.abs(r["c_rotation"][3] - P["idle_frame"]["c_rotation"][3]).max() > 1e-4


def test_oracle_fails_at_entry_for_a_point_on_a_camera_plane():
    p = BO.with_point_on_camera_plane(BO.test_problems()["f3_l1"], 4)
    r = BO.solve(p)
    s = r["summary"]
    assert s["termination"] == "FAILURE" and s["iterations"] == [] and not s["accepted"] and s["final_cost"] == BO.DBL_MAX
    assert np.array_equal(r["position"], p["position"]) and np.array_equal(r["c_rotation"], p["c_rotation"])


def test_boundary_problems_have_the_intended_shapes_and_decide_clear_of_every_threshold(ba):
    G = BO.boundary_problems()
    assert len(G) == len(BO.BOUNDARY_SHAPES)
    sizes = set()
    for (F, l, n), (name, p) in zip(BO.BOUNDARY_SHAPES, G.items()):
        st = ba.plan_stats(p)
        assert st["points"] == n and st["camera_unknowns"] == 6 * F - (6 if l == F - 1 else 9), (name, st)
        assert st["chunk_points"] == 16 and st["row_length"] % 4 == 0 and st["row_length"] >= st["camera_unknowns"] + 1
        sizes.add((st["camera_unknowns"], n))
        if n <= 64:      # (the larger ones are solved by the GPU file, which asserts their margin too)
            s = BO.solve(p)["summary"]
            m = BO.decision_margin(s)
            print("%-14s records %d %-22s margin %.3g (%s, record %d)" % (name, len(s["iterations"]), s["termination"], m[0], m[1], m[2]))
            assert m[0] >= MARGIN and all(i["step"] >= 0 for i in s["iterations"]), (name, m)
    assert {n for _, n in sizes} >= {1, 15, 16, 17, 31, 32, 33, 255, 256, 257, ba.MAX_POINTS}
    assert {nc for nc, _ in sizes} >= {3, 9, 12, 15, 57, 81, 84}


def test_header_functions_are_exported_and_mirrored(ba):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(tcv_sfm_ba[a-z0-9_]*)\s*\(", hdr))
    assert len(declared) == 5, declared
    L = ba.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"libtcv_hip.so does not export {name}"
    assert declared == set(ba.EXPORTS)
    import tcv
    assert not any(n.startswith("tcv_sfm_ba") for n in tcv.EXPORTS)
    assert "tcv_sfm_ba" not in open(os.path.join(ROOT, "include", "tcv.h")).read()
    assert "tcv_sfm_ba" not in open(os.path.join(ROOT, "include", "tcv_estimator.h")).read()
    src = open(os.path.join(ROOT, "tc-viml_amd", "tcv_sfm_ba.py")).read()
    assert "sfm_ba_oracle" not in src and "pose_graph_oracle" not in src and "np_oracle" not in src and "import orc" not in src
    for k, v in (("MAX_FRAMES", ba.MAX_FRAMES), ("MAX_POINTS", ba.MAX_POINTS), ("MAX_BATCH", ba.MAX_BATCH), ("MAX_TRACE", ba.MAX_TRACE)):
        assert re.search(r"#define TCV_SFM_BA_%s %d\b" % (k, v), hdr), k
    assert ba.MAX_FRAMES >= 11 and ba.MAX_POINTS >= 1024 and ba.MAX_TRACE >= 51


def test_header_is_valid_c99_and_cxx14(ba, tmp_path):
    c = os.path.join(tmp_path, "t.c")
    open(c, "w").write('#include "tcv_sfm_ba.h"\nint main(void){ tcv_sfm_ba_options o; tcv_sfm_ba_options_default(&o); '
                       'return (int)sizeof(tcv_sfm_ba_result) > 0 && sizeof(tcv_sfm_ba_desc) > 0 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + inc, "-fsyntax-only", c])
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + inc, "-x", "c++", "-fsyntax-only", c])
    # the mirror's structures have the header's sizes: a C program prints them
    exe = os.path.join(tmp_path, "sizes")
    open(c, "w").write('#include <stdio.h>\n#include "tcv_sfm_ba.h"\nint main(void){ printf("%d %d %d %d\\n", (int)sizeof(tcv_sfm_ba_desc), '
                       '(int)sizeof(tcv_sfm_ba_options), (int)sizeof(tcv_sfm_ba_summary), (int)sizeof(tcv_sfm_ba_result)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I" + inc, c, "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(ba.Desc), C.sizeof(ba.Options), C.sizeof(ba.Summary), C.sizeof(ba.Result)]


def test_defaults_reproduce_the_reference(ba):
    o = ba.default_options()
    D = BO.CERES_DEFAULTS
    assert (o.max_num_iterations, o.max_num_consecutive_invalid_steps, o.accept_cost) == (D["max_num_iterations"], D["max_num_consecutive_invalid_steps"], BO.ACCEPT_COST)
    assert (o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius, o.min_relative_decrease) == \
        (D["function_tolerance"], D["gradient_tolerance"], D["parameter_tolerance"], D["initial_trust_region_radius"], D["min_relative_decrease"])
    assert (o.max_num_iterations, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius) == (50, 1e-6, 1e-10, 1e-8, 1e4)


def run_raw(ba, P, options=None):
    """status of tcv_sfm_ba over Problem objects, and whether every output array and summary is still untouched"""
    rc, out, res = ba.bundle_adjust_raw([p.desc for p in P], options)
    clean = all(not a.any() for o in out for a in o.values()) and all(res[k].summary.iterations == 0 and res[k].summary.termination == 0 for k in range(len(P)))
    return rc, clean


def test_every_validation_error(ba):
    import tcv
    L = ba.lib()
    good = BO.test_problems()["f3_l1"]

    def rc_of(edit=None, **kw):
        p = ba.Problem(dict(good, **kw))      # (a Problem copies the arrays: the edits poke the copies)
        if edit:
            edit(p)
        after_edit = [a.copy() for a in (p.rot, p.tr, p.pos, p.first, p.count, p.frame, p.uv)]
        rc, clean = run_raw(ba, [p])
        assert clean, "an output array was written"
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after_edit, (p.rot, p.tr, p.pos, p.first, p.count, p.frame, p.uv))), "an input array was written"
        return rc

    def setf(**f):
        def e(p):
            for k, v in f.items():
                setattr(p.desc, k, v)
        return e

    def poke(arr, idx, val):
        def e(p):
            getattr(p, arr).reshape(-1)[idx] = val
        return e

    INV = tcv.TCV_ERR_INVALID
    assert rc_of(setf(n_frames=1)) == INV and b"n_frames < 2" in L.tcv_last_error()
    assert rc_of(setf(l=-1)) == INV and b"l out of range" in L.tcv_last_error()
    assert rc_of(setf(l=3)) == INV and b"l out of range" in L.tcv_last_error()
    assert rc_of(setf(n_points=0)) == INV and b"n_points" in L.tcv_last_error()
    for f in ("c_rotation", "c_translation", "position", "obs_first", "obs_count", "obs_frame", "obs_uv"):
        assert rc_of(setf(**{f: None})) == INV and b"missing array" in L.tcv_last_error(), f
    assert rc_of(poke("frame", 3, 3)) == INV and b"frame index out of range" in L.tcv_last_error()
    assert rc_of(poke("frame", 3, -1)) == INV and b"frame index out of range" in L.tcv_last_error()
    assert rc_of(poke("count", 2, 1)) == INV and b"fewer than 2" in L.tcv_last_error()
    assert rc_of(poke("first", 5, 10 ** 6)) == INV and b"observation range" in L.tcv_last_error()
    assert rc_of(poke("first", 5, -1)) == INV and b"observation range" in L.tcv_last_error()

    def twice(p):
        o = int(p.first[0])
        p.frame[o + 1] = p.frame[o]
    assert rc_of(twice) == INV and b"same frame twice" in L.tcv_last_error()
    for arr, val in (("rot", np.nan), ("tr", np.inf), ("pos", -np.inf), ("uv", np.nan)):
        assert rc_of(poke(arr, 1, val)) == INV and b"non-finite" in L.tcv_last_error(), arr
    assert rc_of(c_rotation=np.zeros((3, 4))) == INV and b"zero quaternion" in L.tcv_last_error()
    # the call's own arguments, the result arrays, the options
    p = ba.Problem(good)
    arr = (ba.Desc * 1)(p.desc)
    res = (ba.Result * 1)()
    assert L.tcv_sfm_ba(1, arr, None, res, None) == INV and b"missing result array" in L.tcv_last_error()
    assert L.tcv_sfm_ba(0, arr, None, res, None) == INV
    assert L.tcv_sfm_ba(1, None, None, res, None) == INV
    assert L.tcv_sfm_ba(1, arr, None, None, None) == INV
    assert run_raw(ba, [p], ba.default_options(initial_trust_region_radius=0.0))[0] == INV
    assert run_raw(ba, [p], ba.default_options(function_tolerance=np.nan))[0] == INV
    assert run_raw(ba, [p], ba.default_options(max_num_iterations=-1))[0] == INV
    # the second problem of a batch is validated too
    bad = ba.Problem(good); bad.desc.position = None
    assert run_raw(ba, [p, bad])[0] == INV and b"problem 1" in L.tcv_last_error()
    # observations
    with pytest.raises(tcv.TcvError) as e:
        ba.eval_observations([[0.0, 0, 0, 0]], np.zeros(3), np.ones(3), np.zeros(2))
    assert e.value.status == INV
    with pytest.raises(tcv.TcvError) as e:
        ba.eval_observations([[1.0, 0, 0, 0]], [np.nan, 0, 0], np.ones(3), np.zeros(2))
    assert e.value.status == INV
    assert L.tcv_sfm_ba_eval_observations(1, None, None, None, None, None, None, None) == INV
    assert L.tcv_sfm_ba_plan_stats(None, None) == INV
    assert L.tcv_sfm_ba_last_timing(None) == INV


def big_problem(F, n_points):
    q = np.tile([1.0, 0, 0, 0], (F, 1))
    return dict(c_rotation=q, c_translation=np.zeros((F, 3)), l=0, position=np.tile([0.0, 0, 5.0], (n_points, 1)),
                observations=[[(0, 0.0, 0.0), (1, 0.0, 0.0)] for _ in range(n_points)])


def test_limits_are_unsupported_before_any_launch(ba):
    """beyond the declared limits: TCV_ERR_UNSUPPORTED, with or without a device (the check sits in front of the device test)"""
    import tcv
    L = ba.lib()
    UNS = tcv.TCV_ERR_UNSUPPORTED
    frames = ba.Problem(big_problem(ba.MAX_FRAMES + 1, 4))
    assert run_raw(ba, [frames]) == (UNS, True) and b"TCV_SFM_BA_MAX_FRAMES" in L.tcv_last_error()
    points = ba.Problem(big_problem(3, ba.MAX_POINTS + 1))
    assert run_raw(ba, [points]) == (UNS, True) and b"TCV_SFM_BA_MAX_POINTS" in L.tcv_last_error()
    ok = ba.Problem(BO.test_problems()["f3_l1"])
    assert run_raw(ba, [ok, points]) == (UNS, True)
    assert run_raw(ba, [ok] * (ba.MAX_BATCH + 1)) == (UNS, True) and b"TCV_SFM_BA_MAX_BATCH" in L.tcv_last_error()
    # an invalid problem behind one beyond a limit is still invalid
    bad = ba.Problem(BO.test_problems()["f3_l1"]); bad.desc.l = 7
    assert run_raw(ba, [points, bad])[0] == tcv.TCV_ERR_INVALID
    with pytest.raises(tcv.TcvError) as e:
        ba.plan_stats(frames)
    assert e.value.status == UNS


def test_valid_input_without_a_device_is_no_device(ba):
    import tcv
    if tcv.lib().tcv_device_count() > 0:
        pytest.skip("a HIP device is visible")
    p = ba.Problem(BO.test_problems()["f3_l1"])
    assert run_raw(ba, [p]) == (tcv.TCV_ERR_NO_DEVICE, True)
    with pytest.raises(tcv.TcvError) as e:
        ba.bundle_adjust([BO.test_problems()["f11_l0_p40"]])
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE
    with pytest.raises(tcv.TcvError) as e:
        ba.eval_observations([[1.0, 0, 0, 0]], np.zeros(3), [0.0, 0, 5.0], np.zeros(2))
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE


def test_plan_stats(ba):
    """57 camera unknowns at F = 11 wherever the reference frame lies in front of the last one; the host's column count is the oracle's"""
    for l in (0, 5, 9):
        p = BO.make_problem(50 + l, F=11, n_points=20, l=l)
        st = ba.plan_stats(p)
        G = BO.Problem(p)
        assert st["camera_unknowns"] == 57 == G.nc and st["points"] == 20 and st["observations"] == len(G.ofr)
        assert st["row_length"] == 60 and st["lds_bytes"] == 8 * (256 + 60 * 60 + 48 * 60 + 27 * 11 + 120) and st["lds_bytes"] <= 64 * 1024
        nx, nu = 7 * 11 + 3 * 20, 57 + 3 * 20
        assert st["scratch_bytes"] == 8 * (2 * nx + 2 * nu + 38 * len(G.ofr) + 9 * 20)
    assert ba.plan_stats(BO.make_problem(1, F=11, n_points=5, l=10))["camera_unknowns"] == 60      # l = F - 1: one constant translation fewer
    assert ba.plan_stats(BO.test_problems()["f2_l0"])["camera_unknowns"] == 3
    # observation ranges in any order and with gaps: the host repacks them in point order
    p = ba.Problem(BO.test_problems()["f3_l1"])
    assert ba.plan_stats(p)["observations"] == int(p.count.sum())
