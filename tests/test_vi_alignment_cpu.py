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
