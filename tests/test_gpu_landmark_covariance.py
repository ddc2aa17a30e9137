"""GPU tests of the landmarks' marginal covariance (include/tcv_landmark_covariance.h; phase 7 of tc-viml_amd/csrc/tcv_cov.hip).

Parity gate, per window, for the variances and for the cross rows separately: e(device) <= 8 x max(e(float64 oracle path)) over the
path's two summation orders, and e(device) < 1e-3, against the long-double yardstick of tests/landmark_covariance_oracle.py with
e = |v - vx| / vx for variances and |c - cx| / sqrt(vx_l Cx_jj) for cross entries.  It is the gate of tests/test_gpu_covariance.py, for
its reasons: the phase stands on the same Cholesky factor of S (condition 1e15), a float64 inverse of which is itself off by
1e-6 .. 1e-4, and reordering the float64 sums alone moves that error by up to 2x.  A wrong slot, offset or sign shows at 1e-2 or more.

Measured on an MI355X (profiles/landmark_covariance.txt has the table, 19 rows): worst ratio e(device) / max e(float64 path) 4.04 for
the variances (constant_extrinsic, solved states: 1.66e-6 against 4.11e-7; then golden_prior, initial states, 3.92; every other row
<= 1.36) and 1.65 for the cross rows (golden_prior, initial states); worst e(device) 3.82e-6 (variances, full, solved states) and
6.33e-6 (cross rows, frames4, solved states).

The exact properties are checked bit for bit: run to run, alone against inside a 300-window mixed batch against the reversed batch, the
three getters against each other, the two covariance calls sharing one batch, and that a batch which computes landmark covariances
solves, fixes and marginalises to the same bits as its twin that never does.

No test of a landmark without a point factor: the C-ABI cannot hold one (the header says why), and the CPU test checks the refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_cases as CC
import covariance_oracle as CO
import evaluate_cases as EC
import landmark_covariance_oracle as LO
import synth
import tcv_covariance as cv
import tcv_landmark_covariance as lc

pytestmark = pytest.mark.gpu

CHUNK = 256          # COV_LM_CHUNK of tc-viml_amd/csrc/tcv_cov.h
COMMON = [("pose", -1), ("sb", -1), ("ex", 0), ("pose", 0)]
MIXED = ("frames4", "frames6", "frames6_td", "full", "full_td", "constant_extrinsic", "relocalisation", "golden_prior")


def test_the_chunk_size_of_this_file_is_the_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert re.search(r"COV_LM_CHUNK = %d\b" % CHUNK, open(os.path.join(root, "tc-viml_amd", "csrc", "tcv_cov.h")).read())


def chunk_window(n):
    return synth.window_at(synth.make_windows(610, 1, n_landmarks=n), 0), {}


def case(name):
    if name == "chunk":
        return chunk_window(CHUNK)
    if name == "chunk_plus_1":
        return chunk_window(CHUNK + 1)
    return CC.windows()[name]


_CHUNK_REF = {}


def reference(name, x=None, loss=True, key=None):
    if name in ("chunk", "chunk_plus_1"):
        k = (name, key)
        if k not in _CHUNK_REF:
            _CHUNK_REF[k] = LO.LandmarkReference(CO.Reference(case(name)[0], x))
        return _CHUNK_REF[k]
    return LO.reference(name, x, loss, key)


def hip(gpu, w, kw):
    W, relo = EC.hip_window(gpu, w, **kw)
    if relo is not None:
        W.set_relocalization(relo, 4, np.zeros(3), np.eye(3))
    return W, relo


def device(b, cross, window=0, **kw):
    """(variances, cross rows per block, status of every window) of one window of a batch"""
    lc.compute(b, cross, **kw)
    return lc.variances(b, window), [lc.cross(b, window, k) for k in range(len(cross))], lc.status(b)


def gate(name, tag, R, var, rows, cross):
    e_v, e_v64 = R.e_var(var), R.e_var_f64()
    e_c = max(R.e_cross(c, blk) for c, blk in zip(rows, cross))
    e_c64 = max(R.e_cross_f64(blk) for blk in cross)
    print("landmark parity %-20s %-16s L %3d nc %3d variances e(device) %.2e e(float64 path) %.2e ratio %.3f | cross e(device) %.2e e(float64 path) %.2e ratio %.3f"
          % (name, tag, len(var), R.P.nc, e_v, e_v64, e_v / e_v64, e_c, e_c64, e_c / e_c64))
    assert e_v <= 8 * e_v64 and e_v < 1e-3, (name, tag, "variances", e_v, e_v64)
    assert e_c <= 8 * e_c64 and e_c < 1e-3, (name, tag, "cross", e_c, e_c64)


def same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(u, v) for u, v in zip(a[1], b[1]))


@pytest.mark.parametrize("name", LO.PARITY_CASES + ("chunk", "chunk_plus_1"))
def test_parity_at_the_initial_and_at_the_solved_states(gpu, name):
    w, kw = case(name)
    assert LO.features_in_registration_order(w)
    cross = LO.cross_list(w)
    W, relo = hip(gpu, w, kw)
    b = gpu.Batch([W])
    L = w["lam"].shape[0]
    assert lc.n_landmarks(b, 0) == L
    var, rows, st = device(b, cross)
    assert st[0] == lc.OK and var.shape == (L,) and [r.shape for r in rows] == [(L, lc.SIZES[lc.KINDS[k]]) for k, _ in cross]
    R = reference(name)
    gate(name, "initial", R, var, rows, cross)
    assert same((var, rows), device(b, cross)[:2]), "run to run"
    assert not any(np.any(np.signbit(r[r == 0])) for r in rows), "a zero of this call is +0.0, wherever it comes from"
    if not kw.get("estimate_extrinsic", True):
        assert not np.any(rows[2]) and rows[2].shape == (L, 6)          # a constant cross block: zero rows, as Ceres
    # the bulk getter and the one-problem call return the same bits; the one-problem call by address, in any order
    assert np.array_equal(lc.variances_all(b), var[None, :])
    pick = [L - 1, 0, L // 2]
    v1, r1, st1 = lc.problem(W, pick, cross)
    assert st1 == lc.OK and np.array_equal(v1, var[pick]) and all(np.array_equal(a, c[pick]) for a, c in zip(r1, rows))
    # at the solved states
    b.solve(gpu.default_options(4, True)); b.synchronize(); b.download_states()
    x = EC.oracle_state(R.P, W, relo)
    svar, srows, st = device(b, cross, at_solution=True)
    assert st[0] == lc.OK
    gate(name, "solved", reference(name, x, key="solved"), svar, srows, cross)
    assert not np.array_equal(svar, var)


def test_parity_without_the_loss_function(gpu):
    name = "full"
    w, kw = case(name)
    cross = LO.cross_list(w)
    W, relo = hip(gpu, w, kw)
    b = gpu.Batch([W])
    with_loss = device(b, cross)
    var, rows, st = device(b, cross, apply_loss_function=False)
    assert st[0] == lc.OK and not np.array_equal(with_loss[0], var)
    gate(name, "initial, no loss", reference(name, loss=False), var, rows, cross)


def test_variances_exceed_the_conditional_variance_on_every_landmark(gpu):
    """var(lambda_l) = 1 / H_ll + w'Cw with C positive definite: strictly above the float64 1 / H_ll of the oracle, on every landmark of `full`"""
    W, _ = hip(gpu, *case("full"))
    var, _, st = device(gpu.Batch([W]), [])
    assert st[0] == lc.OK and np.all(var > 1.0 / reference("full").hll64)


def test_alone_inside_a_mixed_batch_and_reversed_same_bits_and_rank_deficient_neighbours(gpu):
    """300 windows of mixed shapes and landmark counts, three of them without a gauge: those report status 1 and all zeros, the call
    returns TCV_OK, and every other window has the bits of its solo run -- in the batch and in the reversed batch"""
    names = list(MIXED)
    wins = [CC.windows()[n] for n in names] + [(CC.no_gauge(s), {}) for s in CC.NO_GAUGE_SEEDS]
    solo = []
    for w, kw in wins:
        W, _ = hip(gpu, w, kw)
        var, rows, st = device(gpu.Batch([W]), COMMON)
        solo.append((var, rows, int(st[0])))
    for k in range(len(names), len(wins)):
        assert solo[k][2] == lc.RANK_DEFICIENT and not np.any(solo[k][0]) and not any(np.any(r) for r in solo[k][1])
    assert all(s == lc.OK and np.all(v > 0) for v, _, s in solo[:len(names)])
    pick = [(7 * i) % len(wins) for i in range(300)]
    keep = [hip(gpu, *wins[p]) for p in pick]
    lmax = max(len(s[0]) for s in solo)
    for order in (list(range(300)), list(range(299, -1, -1))):
        b = gpu.Batch([keep[i][0] for i in order])
        lc.compute(b, COMMON)
        st = lc.status(b)
        allv = lc.variances_all(b)
        assert allv.shape == (300, lmax)
        for pos, i in enumerate(order):
            var, rows, ref_st = solo[pick[i]]
            assert st[pos] == ref_st, (pos, i)
            assert np.array_equal(allv[pos, :len(var)], var) and not np.any(allv[pos, len(var):]), (pos, i)
            assert np.array_equal(lc.variances(b, pos), var)
            for k in range(len(COMMON)):
                assert np.array_equal(lc.cross(b, pos, k), rows[k]), (pos, i, k)


def test_the_two_covariance_calls_share_a_batch_and_keep_their_own_results(gpu):
    """the camera blocks read after a landmark call equal, bit for bit, those of a twin batch that never made one -- and the reverse"""
    w, kw = case("full")
    rq = [(("pose", -1), ("pose", -1)), (("pose", -1), ("sb", -1)), (("ex", 0), ("ex", 0))]

    def batch():
        return gpu.Batch([hip(gpu, w, kw)[0]])
    twin_cv, twin_lc, both = batch(), batch(), batch()
    cv.compute(twin_cv, rq)
    ref_blocks = [cv.block(twin_cv, 0, k) for k in range(len(rq))]
    ref_lm = device(twin_lc, COMMON)
    cv.compute(both, rq)
    lm = device(both, COMMON)
    assert same(lm, ref_lm)
    assert all(np.array_equal(cv.block(both, 0, k), ref_blocks[k]) for k in range(len(rq))) and cv.status(both)[0] == cv.OK      # the earlier call's bits
    cv.compute(both, rq[:2])                                    # another request list replaces the plain call's buffers only
    assert same((lc.variances(both, 0), [lc.cross(both, 0, k) for k in range(len(COMMON))]), ref_lm) and lc.status(both)[0] == lc.OK
    assert np.array_equal(cv.block(both, 0, 1), ref_blocks[1])
    lm2 = device(both, COMMON[:2])                              # and another cross list the landmark call's only
    assert np.array_equal(lm2[0], ref_lm[0]) and np.array_equal(lm2[1][1], ref_lm[1][1])
    assert np.array_equal(cv.block(both, 0, 0), ref_blocks[0])
    # the diagonal of a cross block's own covariance is what the plain call returns: the cross rows are consistent with it (Cauchy-Schwarz)
    cpp = np.diag(ref_blocks[0])
    assert np.all(ref_lm[1][0] ** 2 <= np.outer(ref_lm[0], cpp) * (1 + 1e-9))


def test_the_landmark_call_first_on_a_fresh_batch_then_the_plain_call(gpu):
    """the opposite order of the test above: the slot tables are built on a batch whose owner lists the same call has just made, and
    both results equal, bit for bit, those of twin batches that made only one of the calls"""
    w, kw = case("frames6_td")
    cross = LO.cross_list(w)
    rq = CC.requests("frames6_td")

    def batch():
        return gpu.Batch([hip(gpu, w, kw)[0]])
    twin_cv, twin_lc, both = batch(), batch(), batch()
    cv.compute(twin_cv, rq)
    ref_blocks = [cv.block(twin_cv, 0, k) for k in range(len(rq))]
    ref_lm = device(twin_lc, cross)
    lm = device(both, cross)
    cv.compute(both, rq)
    assert same(lm, ref_lm) and lm[2][0] == ref_lm[2][0] == lc.OK
    assert all(np.array_equal(cv.block(both, 0, k), ref_blocks[k]) for k in range(len(rq))) and cv.status(both)[0] == cv.status(twin_cv)[0] == cv.OK
    assert same((lc.variances(both, 0), [lc.cross(both, 0, k) for k in range(len(cross))]), ref_lm)      # still there behind the plain call


def test_two_plans_in_one_batch_every_window_has_the_bits_of_its_solo_run(gpu):
    """frames4 + frames6_td: the smallest batch in which the second plan's offset is non-zero in the owner lists and in the slot tables"""
    names = ("frames4", "frames6_td")
    solo = [device(gpu.Batch([hip(gpu, *case(n))[0]]), COMMON) for n in names]
    for order in ((0, 1), (1, 0)):
        b = gpu.Batch([hip(gpu, *case(names[i]))[0] for i in order])
        assert b.plan_stats()["num_plans"] == 2
        lc.compute(b, COMMON)
        st = lc.status(b)
        for pos, i in enumerate(order):
            assert st[pos] == solo[i][2][0] == lc.OK, (order, pos)
            assert same((lc.variances(b, pos), [lc.cross(b, pos, k) for k in range(len(COMMON))]), solo[i]), (order, pos)


@pytest.mark.parametrize("setting", ("chain", "dense", "cooperative"))
def test_a_twin_batch_that_never_computes_a_landmark_covariance_ends_with_the_same_bits(gpu, setting):
    wins = [synth.window_at(synth.make_windows(42, 2, frame_shift=-1), k) for k in range(2)]
    gpu.check(gpu.lib().tcv_set_solver_variant(1 if setting == "dense" else 0))
    try:
        res = []
        for with_cov in (False, True):
            W = [gpu.Window(w) for w in wins]
            MW = [gpu.margin_old_window(w) for w in wins]
            M = [gpu.Window(mw, share=W[k]) for k, mw in enumerate(MW)]
            b = gpu.Batch(W, M, [gpu.margin_old_drops(W[k], MW[k]) for k in range(2)])
            if with_cov:
                lc.compute(b, COMMON)
            b.solve(gpu.default_options(6, True, workgroups_per_window=0 if setting == "cooperative" else 1))
            if with_cov:
                lc.compute(b, COMMON, at_solution=True)
            b.gauge_fix()
            if with_cov:
                lc.compute(b, COMMON[:2], at_solution=True)
            b.marginalize()
            if with_cov:
                lc.compute(b, [], at_solution=True)
                assert list(lc.status(b)) == [lc.OK, lc.OK] and np.all(lc.variances(b, 1) > 0)
            b.synchronize(); b.download_states()
            if setting == "cooperative":
                assert b.cooperative()["last_solve_workgroups"] > 1
            assert b.plan_stats()["layout"] == ("dense" if setting == "dense" else "chain")
            res.append((W, bytes(b.summaries()), [b.prior(k).export() for k in range(2)]))
        (Wa, sa, pa), (Wb, sb, pb) = res
        assert sa == sb
        for k in range(2):
            for f in ("pose", "sb", "ex", "lam"):
                assert np.array_equal(getattr(Wa[k], f), getattr(Wb[k], f)), (k, f)
            assert np.array_equal(pa[k]["J0"], pb[k]["J0"]) and np.array_equal(pa[k]["r0"], pb[k]["r0"]) and all(np.array_equal(u, v) for u, v in zip(pa[k]["x0"], pb[k]["x0"]))
    finally:
        gpu.check(gpu.lib().tcv_set_solver_variant(0))


def test_refusals_that_need_a_batch(gpu):
    L = lc.lib()
    Wtd, _ = hip(gpu, *CC.windows()["frames6_td"])
    W6, _ = hip(gpu, *CC.windows()["frames6"])
    b = gpu.Batch([Wtd, W6])
    o = lc.default_options()
    INV = gpu.TCV_ERR_INVALID
    f = L.tcv_batch_compute_landmark_covariance
    arr, n = lc.cross_blocks([("td", 0)])
    assert f(b.h, o, arr, n, None) == INV and b"lacks a requested block" in L.tcv_last_error()      # window 1 has no td
    arr, n = lc.cross_blocks([("pose", 6)])
    assert f(b.h, o, arr, n, None) == INV and b"out of range" in L.tcv_last_error()
    arr, n = lc.cross_blocks([("lam", 0)])
    assert f(b.h, o, arr, n, None) == INV and b"not a landmark" in L.tcv_last_error()
    arr, n = lc.cross_blocks([("pose", -1)])
    assert f(b.h, o, arr, lc.MAX_CROSS + 1, None) == INV and b"n_cross" in L.tcv_last_error()
    assert f(b.h, o, None, 1, None) == INV and b"null cross blocks" in L.tcv_last_error()
    assert f(b.h, None, arr, n, None) == INV and b"null options" in L.tcv_last_error()
    out = np.zeros(64 * 9)
    assert L.tcv_batch_get_landmark_variances(b.h, 0, lc.dptr(out), len(out), None) == INV and b"no landmark covariance has been computed" in L.tcv_last_error()
    o.at_solution = 1
    assert f(b.h, o, arr, n, None) == INV and b"has not been solved" in L.tcv_last_error()
    o.at_solution = 0
    cv.compute(b, [("pose", -1)])                               # a plain covariance call is no landmark call
    assert L.tcv_batch_get_landmark_cross(b.h, 0, 0, lc.dptr(out), len(out), None, None) == INV and b"no landmark covariance has been computed" in L.tcv_last_error()
    gpu.check(f(b.h, o, arr, n, None))
    nl = lc.n_landmarks(b, 0)
    assert L.tcv_batch_get_landmark_variances(b.h, 2, lc.dptr(out), len(out), None) == INV
    assert L.tcv_batch_get_landmark_cross(b.h, 0, 1, lc.dptr(out), len(out), None, None) == INV
    assert L.tcv_batch_get_landmark_variances(b.h, 0, lc.dptr(out), nl - 1, None) == INV and b"too small" in L.tcv_last_error()
    assert L.tcv_batch_get_landmark_cross(b.h, 0, 0, lc.dptr(out), 6 * nl - 1, None, None) == INV and b"too small" in L.tcv_last_error()
    assert L.tcv_batch_get_landmark_variances_all(b.h, lc.dptr(out), 2 * nl - 1, None) == INV and b"too small" in L.tcv_last_error()
    assert not np.any(out)
    st = np.zeros(3, np.int32)
    assert L.tcv_batch_landmark_covariance_status(b.h, lc.iptr(st), 3) == INV
    k = C.c_int(-5)
    assert L.tcv_batch_landmark_covariance_dims(b.h, 2, C.byref(k)) == INV and k.value == -5
    # what is refused as unsupported, through the one-problem call, the caller's arrays untouched.  Both refusals come from the PACKER, inside
    # the call's tcv_batch_create ("projection factor uses one block twice", "4th block must be a free size-1 inverse-depth block"): it meets
    # them before the covariance's own owner-list checks ("covariance: a factor that names one parameter block twice", "covariance: a constant
    # inverse depth"), which stay as a second line behind it and cannot be reached through the C-ABI today.  What is checked here is what a
    # caller sees: TCV_ERR_UNSUPPORTED before any launch, and nothing written.
    w = CC.windows()["frames6"][0]
    twice = gpu.Window(w)
    pi, pj = gpu.f64(w["proj"]["pts_i"][0]).copy(), gpu.f64(w["proj"]["pts_j"][0]).copy()
    gpu.check(L.tcv_problem_add_projection_factor(twice.h, gpu.dptr(pi), gpu.dptr(pj), float(w["proj"]["sqrt_info"]), float(w["proj"]["loss_a"]), twice.block_ptr("pose", 1),
                                                  twice.block_ptr("pose", 1), gpu.dptr(twice.ex), twice.block_ptr("lam", 0)))
    const = gpu.Window(w)
    gpu.check(L.tcv_problem_set_parameter_block_constant(const.h, const.block_ptr("lam", 0)))
    for W, text in ((twice, b"twice"), (const, b"inverse-depth")):
        var = np.full(1, 7.0)
        rc, _, _, s = lc.problem_raw(W, [W.lam.ctypes.data], (), None, var)
        assert rc == gpu.TCV_ERR_UNSUPPORTED and text in L.tcv_last_error() and s == -1 and var[0] == 7.0, (rc, L.tcv_last_error())


def test_landmark_covariance_buffers_go_back_with_the_batch(gpu):
    W = [gpu.Window(synth.window_at(synth.make_windows(5, 2), k)) for k in range(2)]
    live0 = gpu.device_memory_stats()[0]
    b = gpu.Batch(W)
    live1 = gpu.device_memory_stats()[0]
    lc.compute(b, COMMON); lc.variances(b, 1)
    assert gpu.device_memory_stats()[0] > live1
    lc.compute(b, COMMON[:1]); lc.status(b)      # a new cross list replaces the result buffers
    cv.compute(b, [("pose", -1)]); cv.status(b)
    gpu.lib().tcv_batch_destroy(b.h); b.h = None
    assert gpu.device_memory_stats()[0] == live0
    lc.problem(W[0], [0], COMMON[:1])
    assert gpu.device_memory_stats()[0] == live0


def test_ceres_shim_feature_variance(gpu, tmp_path):
    """include/tcv_ceres_shim.hpp tcvshim::Covariance with (feature, feature), (feature, pose) and (pose, feature) pairs: the example"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.LIB_PATH)
    exe = os.path.join(tmp_path, "estimator_shim_classes")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "estimator_shim_classes.cpp"),
                           "-L" + libdir, "-ltcv_hip", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"variance of the feature's inverse depth: (\S+) \(sigma (\S+) at (\S+)\); with the newest pose's x: (\S+); ambient 7 x 1 last entry zero: (\d)", r.stdout)
    assert m, r.stdout
    var, sigma = float(m.group(1)), float(m.group(2))
    assert np.isfinite(var) and var > 0 and abs(sigma * sigma - var) <= 1e-4 * var and np.isfinite(float(m.group(4))) and m.group(5) == "1", r.stdout
