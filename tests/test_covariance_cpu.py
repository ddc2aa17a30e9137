"""CPU side of the batched marginal covariance (include/tcv_covariance.h): the header as C99 / C++14, the ctypes mirror, every refusal
(validated before the device is asked for), the loud failure without a device, and the yardstick of tests/covariance_oracle.py --
that it is at least 100x more accurate than the float64 error it measures, what a float64 path reaches on every test window (printed
for the record: the GPU parity gate is 8x that), that the C oracle's normal matrix gives the same covariance within that band, and the
margins of the rank gate's default.

Figures of this file on the test windows (initial states): float64 Cholesky inverse of a float64 S against the yardstick, two summation
orders: e = 1.3e-6 .. 4.0e-5; yardstick against a 50-digit inverse (nc <= 81): 1000x and more below the float64 error.  Smallest
relative pivot of the well-posed windows 3.6e-11, largest |failing pivot| of the windows without a gauge 2.1e-15; default gate 3e-13
(geometric middle 2.7e-13)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_cases as CC
import covariance_oracle as CO
import synth
from util import sub_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tcv_covariance.h")
CASES = ("frames4", "frames6", "frames6_td", "full", "full_td", "constant_extrinsic", "relocalisation", "golden_prior", "landmarks200")


@pytest.fixture(scope="module")
def cv(built):
    import tcv_covariance
    return tcv_covariance


@pytest.fixture(scope="module")
def tcv(built):
    import tcv
    return tcv


def test_header_functions_are_exported_and_mirrored(cv, tcv):
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(tcv_[a-z_]*covariance[a-z_]*)\s*\(", hdr))
    assert len(declared) == 7, declared
    L = cv.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"libtcv_hip.so does not export {name}"
    assert declared == set(cv.EXPORTS)
    assert not any("covariance" in n for n in tcv.EXPORTS)
    assert "tcv_covariance" not in open(os.path.join(ROOT, "include", "tcv.h")).read() and "TCV_COV" not in open(os.path.join(ROOT, "include", "tcv.h")).read()
    assert "covariance" not in open(os.path.join(ROOT, "include", "tcv_estimator.h")).read().lower()
    src = open(os.path.join(ROOT, "tc-viml_amd", "tcv_covariance.py")).read()
    assert "covariance_oracle" not in src and "np_oracle" not in src and "import orc" not in src
    assert re.search(r"#define TCV_COVARIANCE_MAX_DIM %d\b" % cv.MAX_DIM, hdr) and re.search(r"#define TCV_COVARIANCE_MAX_BLOCKS %d\b" % cv.MAX_BLOCKS, hdr)
    assert float(re.search(r"#define TCV_COVARIANCE_MIN_RELATIVE_PIVOT (\S+)", hdr).group(1)) == cv.MIN_RELATIVE_PIVOT
    for name, v in cv.KINDS.items():
        enum = {"pose": "POSE", "sb": "SPEED_BIAS", "ex": "EXTRINSIC", "td": "TD", "relo": "RELO_POSE", "lam": "LANDMARK"}[name]
        assert re.search(r"TCV_COV_%s = %d\b" % (enum, v), hdr), name
    assert "TCV_ERR_UNSUPPORTED" in hdr and "tangent" in hdr.lower() and "tcv_estimator" in hdr


def test_header_is_valid_c99_and_cxx14_and_the_mirror_has_its_sizes(cv, tmp_path):
    c = os.path.join(tmp_path, "t.c")
    open(c, "w").write('#include "tcv_covariance.h"\nint main(void){ tcv_covariance_options o; tcv_covariance_block b = {TCV_COV_POSE, -1, TCV_COV_SPEED_BIAS, -1}; '
                       'tcv_covariance_options_default(&o); return (int)sizeof(b) > 0 && o.at_solution == 0 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + inc, "-fsyntax-only", c])
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + inc, "-x", "c++", "-fsyntax-only", c])
    exe = os.path.join(tmp_path, "sizes")
    open(c, "w").write('#include <stdio.h>\n#include "tcv_covariance.h"\nint main(void){ printf("%d %d\\n", (int)sizeof(tcv_covariance_options), '
                       '(int)sizeof(tcv_covariance_block)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-I" + inc, c, "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(cv.Options), C.sizeof(cv.Block)] == [16, 16]


def test_the_shim_example_compiles_with_werror_and_exits_0_without_a_device(tcv, tmp_path):
    exe = os.path.join(tmp_path, "estimator_shim_classes")
    libdir = os.path.dirname(tcv.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "estimator_shim_classes.cpp"),
                           "-L" + libdir, "-ltcv_hip", "-Wl,-rpath," + libdir, "-o", exe])
    if tcv.lib().tcv_device_count() == 0:
        assert subprocess.run([exe], capture_output=True, text=True, timeout=120).returncode == 0


def test_defaults(cv):
    o = cv.Options(7, 0, -1.0)
    cv.lib().tcv_covariance_options_default(C.byref(o))
    assert (o.at_solution, o.apply_loss_function, o.min_relative_pivot) == (0, 1, cv.MIN_RELATIVE_PIVOT)
    cv.lib().tcv_covariance_options_default(None)          # NULL: no crash


def test_every_refusal_comes_before_the_device_with_its_message(cv, tcv):
    L = cv.lib()
    w = synth.window_at(synth.make_windows(5, 1), 0)
    W = tcv.Window(w)
    F = w["pose"].shape[0]

    def refused(requests, status, text, options=None, window=W):
        outs = [np.full((9, 9), 7.0) for _ in requests]
        rc, _, st = cv.problem_covariance_raw(window, requests, options, outs)
        assert rc == status, (requests, rc, L.tcv_last_error())
        assert text in L.tcv_last_error(), L.tcv_last_error()
        assert st == -1 and all(np.all(a == 7.0) for a in outs)          # the caller's memory is untouched

    refused([(9, 0)], tcv.TCV_ERR_INVALID, b"unknown block kind")
    refused([(("pose", 0), (-1, 0))], tcv.TCV_ERR_INVALID, b"unknown block kind")
    refused([("pose", F)], tcv.TCV_ERR_INVALID, b"pose index out of range")
    refused([("pose", -F - 1)], tcv.TCV_ERR_INVALID, b"pose index out of range")
    refused([("sb", F)], tcv.TCV_ERR_INVALID, b"speed-bias index out of range")
    refused([("ex", 1)], tcv.TCV_ERR_INVALID, b"index out of range")
    refused([("td", 0)], tcv.TCV_ERR_INVALID, b"lacks a requested block: td")
    refused([("relo", 0)], tcv.TCV_ERR_INVALID, b"lacks a requested block: relocalisation pose")
    refused([("lam", 0)], tcv.TCV_ERR_UNSUPPORTED, b"landmark (inverse depth) blocks are not supported")
    refused([(("pose", -1), ("lam", 3))], tcv.TCV_ERR_UNSUPPORTED, b"landmark")
    refused([("pose", -1)], tcv.TCV_ERR_INVALID, b"min_relative_pivot", cv.default_options(min_relative_pivot=-1.0))
    refused([("pose", -1)], tcv.TCV_ERR_INVALID, b"min_relative_pivot", cv.default_options(min_relative_pivot=float("nan")))
    refused([("pose", -1)], tcv.TCV_ERR_INVALID, b"at_solution", cv.default_options(at_solution=2))
    refused([("pose", -1)], tcv.TCV_ERR_INVALID, b"needs a solved batch", cv.default_options(at_solution=1))
    from evaluate_cases import no_points
    refused([("ex", 0)], tcv.TCV_ERR_INVALID, b"lacks a requested block: extrinsic", window=tcv.Window(no_points(w)))
    # NULL arrays, counts
    o = cv.default_options()
    arr, n = cv.blocks([("pose", -1)])
    out = np.full(36, 7.0)
    ptrs = (C.POINTER(C.c_double) * 1)(cv.dptr(out))
    nul = (C.POINTER(C.c_double) * 1)()
    assert L.tcv_problem_compute_covariance(None, o, arr, n, ptrs, None) == tcv.TCV_ERR_INVALID and b"null problem" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, None, arr, n, ptrs, None) == tcv.TCV_ERR_INVALID and b"null options or blocks" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, o, None, n, ptrs, None) == tcv.TCV_ERR_INVALID and b"null options or blocks" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, o, arr, n, None, None) == tcv.TCV_ERR_INVALID and b"output array" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, o, arr, n, nul, None) == tcv.TCV_ERR_INVALID and b"null output block" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, o, arr, 0, ptrs, None) == tcv.TCV_ERR_INVALID and b"n_blocks" in L.tcv_last_error()
    assert L.tcv_problem_compute_covariance(W.h, o, arr, cv.MAX_BLOCKS + 1, ptrs, None) == tcv.TCV_ERR_INVALID and b"n_blocks" in L.tcv_last_error()
    assert L.tcv_batch_compute_covariance(None, o, arr, n, None) == tcv.TCV_ERR_INVALID and b"null batch" in L.tcv_last_error()
    assert L.tcv_batch_get_covariance(None, 0, 0, cv.dptr(out), 36, None, None) == tcv.TCV_ERR_INVALID
    assert L.tcv_batch_get_covariance_all(None, 0, cv.dptr(out), 36, None, None) == tcv.TCV_ERR_INVALID
    st = np.zeros(1, np.int32)
    assert L.tcv_batch_covariance_status(None, cv.iptr(st), 1) == tcv.TCV_ERR_INVALID
    assert np.all(out == 7.0)


def test_without_a_device_it_is_an_error_and_the_callers_memory_is_untouched(cv, tcv):
    W = tcv.Window(synth.window_at(synth.make_windows(5, 1), 0))
    rq = [("pose", -1), (("pose", -1), ("sb", -1))]
    if tcv.lib().tcv_device_count() > 0:          # run where a device is visible: the call simply works
        outs, st = cv.problem_covariance(W, rq)
        assert st == cv.OK and np.all(np.isfinite(outs[0]))
        return
    before = W.states()
    outs = [np.full((6, 6), 7.0), np.full((6, 9), 7.0)]
    rc, _, st = cv.problem_covariance_raw(W, rq, None, outs)
    assert rc == tcv.TCV_ERR_NO_DEVICE and st == -1 and all(np.all(a == 7.0) for a in outs)
    assert b"no HIP device" in cv.lib().tcv_last_error()
    for k, v in before.items():
        assert np.array_equal(v, W.states()[k])


def test_the_rank_gate_decision_on_the_host_side(cv):
    """tcv_covariance_pivot_status is the function the kernel applies to every pivot: d = L_kk^2, s = S_kk"""
    f = cv.lib().tcv_covariance_pivot_status
    T = cv.MIN_RELATIVE_PIVOT
    assert f(1.0, 1.0, T) == cv.OK and f(2 * T * 3e15, 3e15, T) == cv.OK
    assert f(T * 3e15, 3e15, T) == cv.RANK_DEFICIENT          # at the gate: fails
    assert f(0.5 * T, 1.0, T) == cv.RANK_DEFICIENT and f(0.0, 1.0, 0.0) == cv.RANK_DEFICIENT and f(-1e-3, 1.0, 0.0) == cv.RANK_DEFICIENT
    assert f(1e-300, 1.0, 0.0) == cv.OK
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert f(bad, 1.0, T) == cv.NON_FINITE and f(1.0, bad, T) == cv.NON_FINITE


def test_the_yardstick_is_100x_below_the_float64_error_it_measures():
    """against a 50-digit inverse on windows of at most 5 frames (nc <= 81); on every test window the refinement takes the residual
    |I - S X| of its float64 start down by 100x or more before it stalls"""
    base = synth.window_at(synth.make_windows(9400, 1), 0)
    small = {"frames4": CC.windows()["frames4"][0], "frames5": CC.loose_bias_walk(sub_window(base, 5))}
    for name, w in small.items():
        R = CO.Reference(w)
        assert R.P.nc <= 81
        e_yard = CO.e_full(R.Cx, CO.mp_inverse(R.S))
        print("covariance yardstick %-10s nc %3d e(yardstick vs 50 digits) %.2e e(float64 path) %.2e %.2e: %.0fx below" % (name, R.P.nc, e_yard, R.e_f64[0], R.e_f64[1], min(R.e_f64) / e_yard))
        assert 100 * e_yard <= min(R.e_f64), (name, e_yard, R.e_f64)
    for name in CASES:
        R = CC.reference(name)
        assert len(R.hist) >= 2 and 100 * min(R.hist) <= R.hist[0], (name, R.hist)


def test_what_a_float64_path_reaches_on_the_test_windows_for_the_record():
    """the oracle-only figures the GPU parity gate is built on: float64 cho_solve of a float64 S in two summation orders; the two orders
    stay within 8x of each other (the gate's margin covers a reordering)"""
    for name in CASES:
        R = CC.reference(name)
        print("covariance float64 path %-20s nc %3d e(order 0) %.2e e(order 1) %.2e" % (name, R.P.nc, R.e_f64[0], R.e_f64[1]))
        assert max(R.e_f64) < 1e-3 and max(R.e_f64) <= 8 * min(R.e_f64), (name, R.e_f64)


@pytest.mark.parametrize("name", ("frames6", "full", "golden_prior"))
def test_the_c_oracles_normal_matrix_gives_the_same_covariance_within_the_band(built, name):
    """a second, independent restatement: orc.Window.linearize_dense() assembles H = J'J in C; its Schur complement inverted in float64
    sits in the band of the NumPy float64 path (8x its error)"""
    import orc
    w, kw = CC.windows()[name]
    R = CC.reference(name)
    H, g, cost, n, nc = orc.Window(w).linearize_dense()
    assert n == R.P.nlocal and nc == R.P.nc
    Hn = R.J.T @ R.J
    assert np.abs(H - Hn).max() <= 1e-9 * np.abs(Hn).max()          # the same unknown order
    e = CO.e_full(CO.f64_inverse(CO.schur(H, nc)), R.Cx)
    print("covariance C oracle %-14s e %.2e (NumPy float64 path %.2e %.2e)" % (name, e, R.e_f64[0], R.e_f64[1]))
    assert e <= 8 * max(R.e_f64) and e < 1e-3


def test_the_default_rank_gate_sits_30x_from_every_test_input():
    """smallest relative pivot L_kk^2 / S_kk of the well-posed test windows (in the kernel's elimination order), the pivot at which the
    windows without a gauge fail, the default gate at their geometric middle; every test input 30x away on its side"""
    T = 3e-13
    well = {}
    for name in CASES:
        for loss in (True, False):
            R = CC.reference(name, loss=loss)
            perm = CC.device_order(R.P)
            piv, fail = CO.relative_pivots(np.asarray(R.S, float)[np.ix_(perm, perm)])
            assert fail is None
            well[(name, loss)] = piv.min()
    fails = {}
    for seed in CC.NO_GAUGE_SEEDS:
        P, J, x = CO.linearize(CC.no_gauge(seed))
        perm = CC.device_order(P)
        piv, fail = CO.relative_pivots(CO.reduced_system_f64(P, J, 0)[np.ix_(perm, perm)])
        below = piv[piv <= T]
        first = below[0] if len(below) else fail          # the pivot the gate stops at
        assert first is not None, seed
        passed = piv[:np.argmax(piv <= T)] if len(below) else piv
        fails[seed] = (abs(first), passed.min())
    min_well, max_fail = min(well.values()), max(v[0] for v in fails.values())
    middle = np.sqrt(min_well * max_fail)
    print("covariance rank gate: smallest well-posed pivot %.2e (%s), largest |failing pivot| %.2e, geometric middle %.2e, default %.1e" % (min_well, min(well, key=well.get), max_fail, middle, T))
    assert middle / 1.5 <= T <= middle * 1.5
    assert min_well >= 30 * T and max_fail * 30 <= T
    assert all(v[1] >= 30 * T for v in fails.values()), fails          # what a window without a gauge passes before it fails is far above the gate too
    # the gate the GPU test raises to fail a fine window (1e-8) is 30x above that window's smallest pivot
    assert well[("full", True)] * 30 <= 1e-8
