"""CPU side of the visual-inertial alignment (include/tcv_vi_alignment.h): the NumPy restatement (tests/vi_alignment_oracle.py) recovers
the truth of the generated cases (tests/vi_alignment_cases.py), two and three frames are singular, the rank gate's default lies in the
middle of the measured pivot pair, g2R's invariants, the C-ABI's validation (which runs before the device is touched), the loud failure
without a device, and the header as C99 / C++14."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import synth
import vi_alignment_cases as VC
import vi_alignment_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tcv_vi_alignment.h")
LD = np.longdouble

# the rank gate.  Measured on the restatement, float64, in the kernel's elimination order (natural-order Cholesky), over every input of
# this file and of tests/test_gpu_vi_alignment.py:
SMALLEST_WELL_POSED = 3.5e-8      # smallest relative pivot of a well-posed input (four frames at 50 ms)
LARGEST_SINGULAR = 5.3e-14        # largest |relative pivot| at which a singular input (two or three frames) fails
DEFAULT_GATE = 4e-11              # their geometric middle, 4.3e-11, to one digit
MARGIN = 30.0

WELL_POSED = [(4, 10), (4, 20), (5, 20), (5, 10), (11, 20), (11, 10), (22, 10), (64, 20), (128, 10)]


@pytest.fixture(scope="module")
def va(built):
    import tcv_vi_alignment
    return tcv_vi_alignment


def _angle(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(np.cross(a, b)) / np.linalg.norm(a) / np.linalg.norm(b))


def _errors(r, truth):
    return dict(scale=abs(float(r["scale"]) / truth["scale"] - 1.0), gravity=_angle(r["gravity_c0"], truth["gravity_c0"]),
                bg=float(np.abs(np.asarray(r["bg"], dtype=np.float64) - truth["bg"]).max()))


def test_noise_free_cases_recover_scale_gravity_and_bias():
    """What the float64 restatement leaves, against what the long-double restatement leaves on the same pre-integrations -- the latter is
    the mid-point integrator's error, not rounding.  Measured over WELL_POSED (200 Hz IMU, true bias (0.01, -0.02, 0.015)):
        relative scale error   float64 1.8e-6 .. 1.7e-5    long double the same to 3 digits
        gravity direction      float64 3.9e-7 .. 1.5e-6 rad, long double the same
        gyroscope bias         float64 2.2e-5 .. 2.7e-5,     long double the same
    Gate: float64 <= 10 x long double, per case and quantity."""
    for k, (F, S) in enumerate(WELL_POSED):
        c = VC.make_case(7 + F, F, S)
        r64, _ = VC.run_oracle(c, synth.preintegrate, np.float64)
        rld, _ = VC.run_oracle(c, synth.preintegrate, LD)
        assert r64["status"] == VO.OK and rld["status"] == VO.OK, c["name"]
        e64, eld = _errors(r64, c["truth"]), _errors(rld, c["truth"])
        print("%-24s float64 %s   long double %s" % (c["name"], {k: "%.2e" % v for k, v in e64.items()}, {k: "%.2e" % v for k, v in eld.items()}))
        for q in e64:
            assert e64[q] <= 10.0 * eld[q], (c["name"], q, e64[q], eld[q])
        assert e64["scale"] < 1e-4 and e64["gravity"] < 1e-5 and e64["bg"] < 1e-4, (c["name"], e64)      # and the truth IS recovered
        # the per-frame velocities are the body-frame velocities of the trajectory
        assert np.abs(r64["velocity"] - c["truth"]["velocity"]).max() < 1e-4, c["name"]
        # after the state change gravity is +z at the configured norm and the first key frame has no yaw
        assert np.abs(r64["gravity"] - [0, 0, synth.G_NORM]).max() < 1e-9 and abs(VO.r2ypr(r64["Rs"][0])[0]) < 1e-9, c["name"]


def test_noisy_and_subset_cases_still_align():
    for c in VC.gpu_cases():
        r, _ = VC.run_oracle(c, synth.preintegrate, np.float64, gate=DEFAULT_GATE)
        assert r["status"] == VO.OK, c["name"]
        assert r["Ps"].shape == (len(c["key_frame"]), 3) and np.abs(r["Ps"][0]).max() == 0.0
        e = _errors(r, c["truth"])
        assert e["scale"] < (0.2 if "noisy" in c["name"] else 1e-4), (c["name"], e)


def test_vs_is_indexed_by_kv_as_the_reference_does():
    c = VC.make_case(5, 11, 20, key="sparse")
    r, _ = VC.run_oracle(c, synth.preintegrate)
    kf = c["key_frame"]
    assert list(kf) == [0, 3, 6, 9, 10]
    R0 = r["rot_diff"]
    for kv, i in enumerate(kf):
        assert np.allclose(r["Vs"][kv], R0 @ c["R"][i] @ r["velocity"][kv], rtol=0, atol=1e-15)      # x.segment<3>(3 kv), not 3 i
        assert np.allclose(r["Rs"][kv], R0 @ c["R"][i], rtol=0, atol=1e-15)


def test_two_and_three_frames_are_singular():
    for F in (2, 3):
        for S in (10, 20):
            r, _ = VC.run_oracle(VC.make_case(3 + F, F, S), synth.preintegrate, np.float64, gate=DEFAULT_GATE)
            assert r["status"] == VO.RANK and not r["Ps"].any() and not r["velocity"].any() and r["scale"] == 0
            assert r["delta_bg"] is not None      # the gyroscope bias itself is well-posed from one interval


def _pivot_survey():
    well, sing = [], []
    cases = [VC.make_case(7 + F, F, S) for F, S in WELL_POSED] + VC.gpu_cases()
    for c in cases:
        r, _ = VC.run_oracle(c, synth.preintegrate, np.float64, gate=0.0)
        assert r["status"] == VO.OK, c["name"]
        well.append((float(min(r["pivots"].min(), r["bias_pivots"].min())), c["name"]))
    for F in (2, 3):
        for S in (10, 20):
            for seed in range(4):
                c = VC.make_case(3 + F + 10 * seed, F, S)
                r, _ = VC.run_oracle(c, synth.preintegrate, np.float64, gate=DEFAULT_GATE)
                assert r["status"] == VO.RANK, c["name"]
                sing.append((abs(float(r["pivots"][-1])), c["name"]))
    return min(well), max(sing)


def test_rank_gate_default_sits_between_the_measured_pivots(va):
    (lo, lo_name), (hi, hi_name) = _pivot_survey()
    print("smallest well-posed relative pivot %.3g (%s), largest singular |relative pivot| %.3g (%s), geometric middle %.3g" % (lo, lo_name, hi, hi_name, np.sqrt(lo * hi)))
    assert va.default_options().min_relative_pivot == DEFAULT_GATE
    assert lo >= MARGIN * DEFAULT_GATE and hi <= DEFAULT_GATE / MARGIN, (lo, hi)
    # the recorded pair is what is measured (to rounding of the record), and the default is its geometric middle to one digit
    assert 0.9 * SMALLEST_WELL_POSED <= lo <= 1.1 * SMALLEST_WELL_POSED and 0.5 * LARGEST_SINGULAR <= hi <= 1.1 * LARGEST_SINGULAR, (lo, hi)
    assert 0.9 <= DEFAULT_GATE / np.sqrt(SMALLEST_WELL_POSED * LARGEST_SINGULAR) <= 1.1
    assert va.default_options().gravity_norm == 9.81007


def test_g2R_invariants():
    """R0 g is parallel to +z, and the yaw of R0 Rs[0] is zero after the correction of estimator.cpp:1428-1429 -- also for gravity within
    1e-13 of -z, where FromTwoVectors takes its antiparallel branch with the fixed axis"""
    rng = np.random.default_rng(3)
    gs = [rng.normal(size=3) * 9.8 for _ in range(20)] + [np.array([0, 0, 9.81]), np.array([0, 0, -9.81]), np.array([1e-13, -5e-14, -1.0]) * 9.81,
                                                           np.array([3e-7, 0, -1.0]), np.array([1e-3, 1e-3, -1.0])]
    for g in gs:
        for dt in (np.float64, LD):
            g = g.astype(dt)
            R0 = VO.g2R(g)
            c = float(g[2] / np.sqrt(g @ g))
            # Regular branch: w comes from sqrt(2 (1 + c)), and 1 + c cancels -- the quaternion is off unit length by about eps / (1 + c), and Eigen's
            # toRotationMatrix does not normalise (the reference has the same property).  Antiparallel branch (c < -1 + 1e-12, within 1.4e-6 rad of
            # -z): the quaternion is unit, but the rotation by pi about the fixed axis x maps g to +z only up to twice g's own tilt from -z: 2e-13
            # for the inputs within 1e-13, 6e-7 for the one at 3e-7.
            anti = c < -1.0 + 1e-12
            tol = (1e-6 if abs(float(g[0])) == 3e-7 else 1e-12) if anti else 1e-14 + 8 * 2.2e-16 / (1.0 + c)
            assert np.abs(R0 @ R0.T - np.eye(3)).max() < (1e-14 if anti else tol)
            z = R0 @ g / np.sqrt(g @ g)
            assert abs(float(z[2]) - 1.0) < tol and np.abs(z[:2]).max() < tol, (g, z)
            assert abs(float(VO.r2ypr(R0)[0])) < 1e-9
            Rs0 = synth.q2R(np.array([0.3, -0.2, 0.5, 0.79]) / np.linalg.norm([0.3, -0.2, 0.5, 0.79])).astype(dt)
            yaw = VO.r2ypr(R0 @ Rs0)[0]
            R1 = VO.ypr2R(np.array([-yaw, 0, 0], dtype=dt)) @ R0
            assert abs(float(VO.r2ypr(R1 @ Rs0)[0])) < 1e-9
            z = R1 @ g / np.sqrt(g @ g)
            assert abs(float(z[2]) - 1.0) < tol


def test_header_functions_are_exported_and_mirrored(va):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(tcv_vi_align[a-z0-9_]*)\s*\(", hdr))
    assert declared == {"tcv_vi_align", "tcv_vi_align_options_default", "tcv_vi_align_last_timing"}, declared
    L = va.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"libtcv_hip.so does not export {name}"
    assert declared == set(va.EXPORTS)
    import tcv
    assert not any(n.startswith("tcv_vi_align") for n in tcv.EXPORTS)
    assert "tcv_vi_align" not in open(os.path.join(ROOT, "include", "tcv.h")).read()
    src = open(os.path.join(ROOT, "tc-viml_amd", "tcv_vi_alignment.py")).read()
    assert "vi_alignment_oracle" not in src and "vi_alignment_cases" not in src and "np_oracle" not in src and "import orc" not in src
    for k, v in (("MAX_FRAMES", va.MAX_FRAMES), ("MAX_BATCH", va.MAX_BATCH)):
        assert re.search(r"#define TCV_VI_ALIGN_%s %d\b" % (k, v), hdr), k
    assert (va.MAX_FRAMES, va.MAX_BATCH) == (128, 4096)
    assert (va.OK, va.LINEAR, va.REFINED_SCALE, va.RANK, va.NON_FINITE) == (VO.OK, VO.LINEAR, VO.REFINED_SCALE, VO.RANK, VO.NON_FINITE) == (0, 1, 2, 3, 4)


def test_header_is_valid_c99_and_cxx14(va, tmp_path):
    c = os.path.join(tmp_path, "t.c")
    open(c, "w").write('#include "tcv_vi_alignment.h"\nint main(void){ tcv_vi_align_options o; tcv_vi_align_options_default(&o); '
                       'return (int)sizeof(tcv_vi_align_result) > 0 && sizeof(tcv_vi_align_desc) > 0 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + inc, "-fsyntax-only", c])
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + inc, "-x", "c++", "-fsyntax-only", c])
    exe = os.path.join(tmp_path, "sizes")
    open(c, "w").write('#include <stdio.h>\n#include "tcv_vi_alignment.h"\nint main(void){ printf("%d %d %d\\n", (int)sizeof(tcv_vi_align_desc), '
                       '(int)sizeof(tcv_vi_align_options), (int)sizeof(tcv_vi_align_result)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I" + inc, c, "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(va.Desc), C.sizeof(va.Options), C.sizeof(va.Result)]


def test_every_validation_error(va):
    import tcv
    L = va.lib()
    good = VC.make_case(1, 5, 10)
    INV, UNS = tcv.TCV_ERR_INVALID, tcv.TCV_ERR_UNSUPPORTED

    def rc_of(edit=None, res_edit=None, options=None):
        s = va.Sequence(copy.deepcopy(good))      # (a Sequence shares the arrays it is given: the edits poke)
        if edit:
            edit(s)
        n = 1
        arr = (va.Desc * n)(s.desc)
        res = (va.Result * n)()
        o = va.Outputs(max(s.desc.n_frames, 1), max(s.desc.n_key, 1), False)
        o.bind(res[0])
        if res_edit:
            res_edit(res[0])
        return L.tcv_vi_align(n, arr, C.byref(options) if options is not None else None, res, None)

    def setf(**f):
        def e(s):
            for k, v in f.items():
                setattr(s.desc, k, v)
        return e

    def poke(arr, idx, val):
        def e(s):
            getattr(s, arr).reshape(-1)[idx] = val
        return e

    for F in (1, 0, -3):
        assert rc_of(setf(n_frames=F)) == INV and b"n_frames < 2" in L.tcv_last_error()
    for f in ("R", "T", "first", "count", "samples7", "acc0_gyr0", "key_frame"):
        assert rc_of(setf(**{f: None})) == INV and b"missing array" in L.tcv_last_error(), f
    for f in ("velocity", "Ps", "Rs", "Vs"):
        assert rc_of(res_edit=lambda r, f=f: setattr(r, f, None)) == INV and b"missing result array" in L.tcv_last_error(), f
    assert rc_of(setf(num_samples=-1)) == INV
    assert rc_of(poke("count", 2, 0)) == INV and b"interval without samples" in L.tcv_last_error()
    assert rc_of(poke("first", 1, -1)) == INV and b"out of bounds" in L.tcv_last_error()
    assert rc_of(poke("first", 3, 31)) == INV and b"out of bounds" in L.tcv_last_error()      # 31 + 10 > 40 samples
    assert rc_of(setf(n_key=0)) == INV and rc_of(setf(n_key=6)) == INV and b"n_key" in L.tcv_last_error()
    assert rc_of(poke("key", 1, 1 - 1)) == INV and b"strictly ascending" in L.tcv_last_error()      # 0, 0, ...
    assert rc_of(poke("key", 2, 1)) == INV and b"strictly ascending" in L.tcv_last_error()
    assert rc_of(poke("key", 4, 5)) == INV and b"key_frame out of range" in L.tcv_last_error()
    assert rc_of(poke("key", 0, -1)) == INV and b"key_frame out of range" in L.tcv_last_error()
    for arr, val in (("R", np.nan), ("T", np.inf), ("samples", np.nan), ("init", -np.inf)):
        assert rc_of(poke(arr, 7, val)) == INV and b"non-finite" in L.tcv_last_error(), arr
    for f in ("tic", "ba0", "bg0", "noise"):
        def e(s, f=f):
            getattr(s.desc, f)[1] = float("nan")
        assert rc_of(e) == INV and b"non-finite" in L.tcv_last_error(), f
    for o in (va.default_options(gravity_norm=0.0), va.default_options(gravity_norm=float("nan")), va.default_options(min_relative_pivot=-1e-3),
              va.default_options(min_relative_pivot=1.0), va.default_options(min_relative_pivot=float("nan"))):
        assert rc_of(options=o) == INV and b"options" in L.tcv_last_error()
    # the call's own arguments
    s = va.Sequence(good)
    arr = (va.Desc * 1)(s.desc)
    res = (va.Result * 1)()
    va.Outputs(5, 5, False).bind(res[0])
    assert L.tcv_vi_align(0, arr, None, res, None) == INV
    assert L.tcv_vi_align(1, None, None, res, None) == INV
    assert L.tcv_vi_align(1, arr, None, None, None) == INV
    assert L.tcv_vi_align_last_timing(None) == INV
    # the second sequence of a batch is validated too
    bad = va.Sequence(good); bad.desc.T = None
    assert va.align_raw([s.desc, bad.desc])[0] == INV and b"sequence 1" in L.tcv_last_error()


def test_limits_are_unsupported_before_any_launch(va):
    """beyond the declared limits: TCV_ERR_UNSUPPORTED, with or without a device (the checks sit in front of the device test)"""
    import tcv
    L = va.lib()
    big = va.Sequence(VC.make_case(2, va.MAX_FRAMES + 1, 10, key="one"))
    assert va.align_raw([big.desc])[0] == tcv.TCV_ERR_UNSUPPORTED and b"TCV_VI_ALIGN_MAX_FRAMES" in L.tcv_last_error()
    ok = va.Sequence(VC.make_case(1, 5, 10))
    assert va.align_raw([ok.desc, big.desc])[0] == tcv.TCV_ERR_UNSUPPORTED
    bad = va.Sequence(VC.make_case(1, 5, 10)); bad.desc.R = None
    assert va.align_raw([big.desc, bad.desc])[0] == tcv.TCV_ERR_INVALID      # invalid input wins over a limit
    assert va.align_raw([ok.desc] * (va.MAX_BATCH + 1))[0] == tcv.TCV_ERR_UNSUPPORTED and b"TCV_VI_ALIGN_MAX_BATCH" in L.tcv_last_error()


def test_valid_input_without_a_device_is_no_device(va):
    import tcv
    if tcv.lib().tcv_device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(tcv.TcvError) as e:
        va.align([VC.make_case(1, 5, 10)])
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE


def test_scope_comment_points_at_the_header():
    assert "tcv_vi_alignment.h" in open(os.path.join(ROOT, "include", "tcv_estimator.h")).read()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs off the well-posed path (tests/vi_alignment_cases.py): the restatement alone must be decisive on each of them, in float64 and in
# long double, before tests/test_gpu_vi_alignment_paths.py runs them on the device.
# ---------------------------------------------------------------------------------------------------------------------------------------
from vi_alignment_cases import RANK_SITES, SINGULAR_FRAMES, STATUS2, TILTED, VERTICAL      # noqa: E402  (shared with the GPU tests)

assert VC.DEFAULT_GATE == DEFAULT_GATE


def _both(case, gate=DEFAULT_GATE):
    return VC.run_oracle_imu(case, dtype=np.float64, gate=gate)[0], VC.run_oracle_imu(case, dtype=LD, gate=gate)[0]


def _all_pivots(r):
    return np.concatenate([np.asarray(r["bias_pivots"], dtype=np.float64)] + [np.asarray(p, dtype=np.float64) for _, p in r["stages"]])


@pytest.mark.parametrize("F,S,sign", VERTICAL)
def test_vertical_gravity_takes_the_exact_branches(F, S, sign):
    """gravity exactly along +-z of the SfM frame: TangentBasis's special branch in all four rounds (at -z too -- there the reference's own basis
    is the zero vector), g2R at c == +-1 exactly, the x / y gravity exactly zero"""
    c = VC.vertical_case(F, S, sign)
    for r in _both(c):
        assert r["status"] == VO.OK, (c["name"], r["status"])
        assert r["flags"].get("tangent_special") == 4 and r["flags"]["g2R_c"] == sign
        assert bool(r["flags"].get("g2R_antiparallel")) == (sign < 0)
        assert float(_all_pivots(r).min()) >= MARGIN * DEFAULT_GATE
        assert abs(float(r["scale"]) / c["truth"]["scale"] - 1.0) < 1e-3      # (the mid-point integrator's error on a 3 Hz sine at 4 frames)
    r64 = _both(c)[0]
    print("%-24s smallest relative pivot %.3g, scale %.9f" % (c["name"], float(_all_pivots(r64).min()), float(r64["scale"])))
    assert r64["gravity_c0"][0] == 0 and r64["gravity_c0"][1] == 0 and r64["gravity_c0"][2] == sign * 9.81007
    assert not r64["delta_bg"].any()
    if sign < 0:      # the rotation by pi about x (the yaw correction is exactly zero: Rs[0] = diag(1, -1, -1))
        assert np.abs(r64["rot_diff"] - np.diag([1.0, -1.0, -1.0])).max() < 1e-15 and np.abs(r64["gravity"] - [0, 0, 9.81007]).max() < 1e-14


@pytest.mark.parametrize("F,S,delta", TILTED)
def test_tilted_gravity_is_on_the_intended_side_of_the_antiparallel_threshold(F, S, delta):
    c = VC.tilted_case(F, S, delta)
    for r in _both(c):
        assert r["status"] == VO.OK and not r["flags"].get("tangent_special")
        cc = r["flags"]["g2R_c"]
        print("%-22s %s 1 + c = %.3e" % (c["name"], r["scale"].dtype, float(1 + cc)))
        assert bool(r["flags"].get("g2R_antiparallel")) == (delta < 1e-6)
        # and clear of the threshold 1e-12 by 100 x: 1 + c = delta^2 / 2 = 5e-15 | 5e-5
        assert float(1 + cc) < 1e-14 if delta < 1e-6 else float(1 + cc) > 1e-10
        assert _angle(r["gravity_c0"], c["truth"]["gravity_c0"]) < 1e-5


def test_refined_scale_seeds_are_decided_by_more_than_rounding():
    """status 2: LinearAlignment's s >= 0, the refined s < 0, in float64 and long double; |s| at both stages >= 100 x its float64-to-long-double
    difference"""
    assert len(STATUS2) >= 3
    for seed, F in STATUS2:
        c = VC.noise_T_case(seed, F)
        r64, rld = _both(c)
        assert r64["status"] == rld["status"] == VO.REFINED_SCALE, (c["name"], r64["status"], rld["status"])
        for stage, a, b in (("linear", r64["linear"]["scale"], rld["linear"]["scale"]), ("refined", r64["scale"], rld["scale"])):
            d = abs(float(LD(a) - b))
            print("%-20s %-8s s %+.4e   |float64 - long double| %.2e   bar %.2e" % (c["name"], stage, float(a), d, 100 * d))
            assert abs(float(a)) >= 100 * d, (c["name"], stage)
        assert r64["linear"]["scale"] >= 0 > r64["scale"] and r64["velocity"].any() and not r64["Ps"].any()
        assert float(_all_pivots(r64).min()) >= MARGIN * DEFAULT_GATE


def _sites(case):
    """every recorded relative pivot of a case at gate 0, in the order the device meets them, with its site"""
    r = VC.run_oracle_imu(case, gate=0.0)[0]
    F = len(case["R"])
    seq = [("bias", float(p)) for p in r["bias_pivots"]]
    for stage, piv in r["stages"]:
        seq += [("band" if j < 3 * F else "linear border" if stage == "linear" else "refine border", float(p)) for j, p in enumerate(piv)]
    return seq


def _gates_by_site(seq):
    vals = sorted({p for _, p in seq})
    out = {}
    for lo, hi in zip(vals[:-1], vals[1:]):
        g = float(np.sqrt(lo * hi))
        if lo > 0 and hi / lo >= MARGIN ** 2 and g < 1.0:
            out.setdefault(next(s for s, p in seq if not p > g), []).append((g, lo, hi))
    return out


def test_rank_gate_sites_reachable_from_well_posed_input():
    """Status 3 site by site: a min_relative_pivot in the geometric middle of two neighbouring recorded pivots >= 30^2 apart, so that both are 30 x
    clear of it; the site is where the first failing pivot falls.

    Reachable: LinearAlignment's border (nb == 4), on four and five frames at 50 ms -- RANK_SITES.
    NOT reachable this way, searched over WELL_POSED, vertical_case (F 4 | 11, both signs), tilted_case (1e-7, 1e-2), ragged_case (three seeds)
    and the STATUS2 seeds:
      - the bias kernel's 3 x 3: its relative pivots are 1 to three digits (J is -sum_dt I to first order), nothing lies 30 x under 1.  The
        exactly singular zero_dt_case (below) reaches that site and the alignment kernel's early exit at the default gate;
      - a band pivot: the band's pivots lie in 0.04 .. 1 (the velocity block is dt^2 I plus a chain), above every border pivot of the same case,
        and no two neighbours are 900 x apart;
      - the border of a RefineGravity round (nb == 3, index map 0 1 3): its smallest pivot is always above LinearAlignment's smallest (two
        gravity directions are eliminated before the scale, not three), so a gate that fails it fails LinearAlignment first.  Before the
        TangentBasis fix vertical_case(sign = -1) failed exactly there, with A_kk == 0.  The index map itself runs in every aligned case."""
    found = {}
    for F, S in WELL_POSED:
        for site, gs in _gates_by_site(_sites(VC.make_case(7 + F, F, S))).items():
            found.setdefault(site, []).extend((F, S) + g for g in gs)
    others = [VC.vertical_case(F, S, sg) for F, S, sg in VERTICAL] + [VC.tilted_case(*t) for t in TILTED] + [VC.ragged_case(k, F) for k, F in enumerate((6, 23, 65))] + \
        [VC.noise_T_case(seed, F) for seed, F in STATUS2]
    for c in others:
        assert not _gates_by_site(_sites(c)), c["name"]
    for site, gs in found.items():
        for F, S, g, lo, hi in gs:
            print("%-14s F %d period %d: gate %.3g between the pivots %.3g and %.3g" % (site, F, S, g, lo, hi))
    assert set(found) == {"linear border"}
    assert sorted((F, S) for F, S, _, _, _ in found["linear border"]) == sorted((F, S) for F, S, _, _ in RANK_SITES)
    for F, S, gate, site in RANK_SITES:
        g, lo, hi = next(x[2:] for x in found[site] if x[:2] == (F, S))
        assert abs(gate / g - 1.0) < 0.01 and lo * MARGIN <= gate <= hi / MARGIN
        c = VC.make_case(7 + F, F, S)
        del c["period"]
        for r in _both(c, gate):
            assert r["status"] == VO.RANK and r["site"] == site and r["delta_bg"].any() and not r["velocity"].any() and r["scale"] == 0


@pytest.mark.parametrize("F", SINGULAR_FRAMES)
def test_exactly_singular_inputs_fail_the_gate_clearly(F):
    """a camera at rest (T == 0: the scale column is exactly zero, A_kk == 0 at the failing pivot), constant velocity without rotation (scale and a
    common velocity confounded: |relative pivot| at the failure <= DEFAULT_GATE / MARGIN), and IMU samples with dt == 0 (the bias Jacobians are
    exactly zero: the bias solve itself fails, on A_00 == 0, and nothing behind it is computed)"""
    for r in _both(VC.stationary_case(F)):
        assert r["status"] == VO.RANK and r["site"] == "linear border" and r["fail_a0"] == 0 and len(r["stages"][0][1]) == 3 * F + 4
        assert r["delta_bg"].any()
    for r in _both(VC.constant_velocity_case(F)):
        print("constant velocity F %d: relative pivot at the failure %.3g (%s)" % (F, float(r["pivots"][-1]), r["scale"].dtype))
        assert r["status"] == VO.RANK and r["site"] == "linear border" and abs(float(r["pivots"][-1])) <= DEFAULT_GATE / MARGIN
        assert r["min_pivot"] >= MARGIN * DEFAULT_GATE
    for r in _both(VC.zero_dt_case(F)):
        assert r["status"] == VO.RANK and r["site"] == "bias" and r["fail_a0"] == 0 and not r["delta_bg"].any() and not r["bg"].any()


def test_scaling_T_alone_never_gives_non_finite():
    """|T| scaled by 10^k: the float64 restatement is OK for k in -150 .. 152 (s = 2.43 x 10^-k, finite), and RANK outside -- below, the squares
    of the scale column underflow to an A_kk of zero or a denormal; above, they overflow and the pivot test `d > gate * A_kk` is false for Inf
    and NaN.  The matrix is shielded by the gate; the right-hand side is not (next test)."""
    c = VC.make_case(18, 11, 20)
    seen = {}
    for k in (-320, -300, -200, -160, -150, -100, 0, 100, 152, 156, 200, 300):
        cc = dict(c, T=c["T"] * 1e-160 * 10.0 ** (k + 160) if k < -160 else c["T"] * 10.0 ** k)
        del cc["period"]
        assert np.isfinite(cc["T"]).all()
        seen[k] = int(VC.run_oracle_imu(cc, gate=DEFAULT_GATE)[0]["status"])
    print(seen)
    assert all(seen[k] == VO.OK for k in (-150, -100, 0, 100, 152)) and all(seen[k] == VO.RANK for k in (-320, -300, -200, -160, 156, 200, 300))


@pytest.mark.filterwarnings("ignore::RuntimeWarning")      # (the overflows are the point: synth.preintegrate's covariance, the products of the right-hand side)
def test_non_finite_after_linear_alignment_from_a_huge_accelerometer():
    """Status 4, site by site.

    After LinearAlignment's s, g -- REACHED: huge_acc_case(k, 100), accelerometer x 10^k on T x 10^100, every input finite.  The matrices do not
    depend on the accelerometer, so every pivot is that of the plain case; delta_p and delta_v scale with it, and their products with the scale
    column overflow.  Float64 restatement at the default gate: LINEAR with finite s = 2.46 x 10^(k - 100) and |g| = 9.81 x 10^k for k <= 208,
    NON_FINITE for k >= 209 up to 300.  Committed: k = 212 (NON_FINITE) and k = 206 (LINEAR), more than two decades on either side.  Long
    double does not overflow there and says LINEAR: the verdict is one about float64's range, which the device shares.  (With T unscaled the
    same happens between k = 305 and 306, but at k = 307 the mid-point sum of two samples overflows inside the pre-integration itself.)
    After the refinement's s, g, x -- NOT reached: it needs LinearAlignment finite with | |g| - G | <= 1 and s >= 0, then an overflow one solve
    later in a system that differs by g0's terms only; every input with a right-hand side large enough to overflow has |g| large and ends in
    LINEAR (all of the above), and a gravity_norm large enough to accept it would need |g| to hit it within 1, below float64's spacing there.
    After the bias solve -- NOT reached: J is -sum_dt I to first order and |r| <= 2, so delta_bg is about r / dt; swept with every dt = 10^k: finite
    (2.5 x 10^159 at k = -162) down to k = -162, RANK on A_00 == 0 from k = -165, where dt^2 underflows -- measured below."""
    seen = {}
    for k in (150, 200, VC.LINEAR_SIDE_K, 207, 208, 209, 210, 211, VC.NON_FINITE_K, 250, 300):
        c = VC.huge_acc_case(k)
        assert all(np.isfinite(m[0]).all() and np.isfinite(m[2]).all() for m in c["imu"]) and np.isfinite(c["T"]).all()
        r = VC.run_oracle_imu(c, gate=DEFAULT_GATE)[0]
        seen[k] = int(r["status"])
        if r["status"] == VO.LINEAR:
            assert np.isfinite(float(r["scale"])) and np.isfinite(np.asarray(r["gravity_c0"], dtype=np.float64)).all() and r["scale"] > 0
        else:      # the header's zero pattern: the bias and the pre-integrations stay, nothing behind them
            assert r["delta_bg"].any() and not any(np.asarray(r[f]).any() for f in ("scale", "gravity_c0", "gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"))
        assert r["min_pivot"] >= MARGIN * DEFAULT_GATE and len(r["stages"]) == 1      # every pivot passed; nothing ran behind LinearAlignment
    print(seen)
    assert all(seen[k] == VO.LINEAR for k in seen if k <= 208) and all(seen[k] == VO.NON_FINITE for k in seen if k >= 209)
    assert VC.LINEAR_SIDE_K <= 208 - 2 and VC.NON_FINITE_K >= 209 + 2
    assert VC.run_oracle_imu(VC.huge_acc_case(VC.NON_FINITE_K), dtype=LD, gate=DEFAULT_GATE)[0]["status"] == VO.LINEAR
    # the bias site under tiny dt
    c0 = VC.make_case(18, 11, 20)
    for k, want in ((-100, VO.OK), (-150, VO.OK), (-162, VO.OK), (-165, VO.RANK), (-200, VO.RANK), (-300, VO.RANK)):
        imu = [(a0, g0, np.concatenate([np.full((len(s), 1), 10.0 ** k), s[:, 1:]], 1)) for a0, g0, s in c0["imu"]]
        st, x, _, a0 = VO.gyro_bias_verdict(c0["R"], VC.preint_np(imu, c0["ba0"], c0["bg0"]), np.float64, DEFAULT_GATE)
        print("dt 1e%d: bias status %d, |delta_bg| %.3g" % (k, st, float(np.abs(x).max())))
        assert st == want and np.isfinite(np.asarray(x, dtype=np.float64)).all() and (st == VO.OK or a0 == 0)


def test_negated_T_is_status_1_by_the_sign_of_s():
    c = VC.negated_T_case()
    for r in _both(c):
        assert r["status"] == VO.LINEAR and abs(float(r["scale"]) + c["truth"]["scale"]) < 1e-3 * c["truth"]["scale"]
        assert abs(float(np.sqrt(r["gravity_c0"] @ r["gravity_c0"])) - 9.81007) < 0.5 and float(_all_pivots(r).min()) >= MARGIN * DEFAULT_GATE


def test_ragged_cases_align_and_skip_frame_zero():
    for k, F in enumerate((6, 23, 65)):
        c = VC.ragged_case(k, F)
        counts = [len(m[2]) for m in c["imu"]]
        assert min(counts) >= 3 and max(counts) <= 40 and len(set(counts)) > 1 and 0 not in c["key_frame"]
        assert all(len({float(v) for v in m[2][:, 0]}) > 1 for m in c["imu"]) and {float(v) for m in c["imu"] for v in m[2][:, 0]} == {0.0025, 0.005, 0.01}
        r64, rld = _both(c)
        assert r64["status"] == rld["status"] == VO.OK and float(_all_pivots(r64).min()) >= MARGIN * DEFAULT_GATE
        e = _errors(r64, c["truth"])
        assert e["scale"] < 1e-4 and e["gravity"] < 1e-5 and e["bg"] < 1e-4, (c["name"], e)


def test_dense_solve_agrees_with_the_cholesky():
    """the second float64 solve (numpy.linalg.solve) gives the Cholesky's answer up to rounding: it sizes noise, it is not another algorithm"""
    for F, S in ((4, 10), (11, 20), (64, 20)):
        c = VC.make_case(7 + F, F, S)
        del c["period"]
        a = VC.run_oracle_imu(c)[0]; b = VC.run_oracle_imu(c, solver="dense")[0]; ld = VC.run_oracle_imu(c, dtype=LD)[0]
        assert b["status"] == VO.OK
        for f in ("delta_bg", "scale", "gravity_c0", "velocity", "Ps"):
            ea, eb = float(np.abs(a[f] - ld[f]).max()), float(np.abs(b[f] - ld[f]).max())
            print("F %3d %-10s |cholesky - long double| %.2e   |linalg.solve - long double| %.2e" % (F, f, ea, eb))
            assert eb <= 1e-6 * max(float(np.abs(ld[f]).max()), 1e-3)      # (condition numbers to 9e12 at four frames: 1e-16 x that, 1000 x spare)


def test_fuzz_seed_range_is_decided_by_the_restatement_alone():
    """tests/dev/fuzz_vi_alignment.py, the suite's seeds 0 .. 59 on the CPU's pre-integrations: at most 5 % undecided (measured: 0 of 60; 0 of
    300 over seeds 0 .. 299)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "dev"))
    try:
        import fuzz_vi_alignment as FZ
    finally:
        sys.path.remove(os.path.join(ROOT, "tests", "dev"))
    left = []
    for seed in range(60):
        c = VC.fuzz_case(seed)
        r64, rld, _ = FZ.reference(c, with_dense=False)
        why = FZ.undecided(r64, rld)
        if why:
            left.append((c["name"], why))
    print("left out on the CPU: %d of 60 %s" % (len(left), left))
    assert len(left) <= FZ.MAX_LEFT_OUT * 60
    assert (FZ.GATE, FZ.MARGIN) == (DEFAULT_GATE, MARGIN)
