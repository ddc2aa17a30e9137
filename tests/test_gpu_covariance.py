"""GPU tests of the batched marginal covariance (include/tcv_covariance.h; tc-viml_amd/csrc/tcv_cov.hip).

Parity gate, per window: e(device) <= 8 x max(e(float64 oracle path)) over the window's two summation orders, and e(device) < 1e-3,
with e = max |C - Cx| / sqrt(Cx_ii Cx_jj) over the requested blocks against the long-double yardstick of tests/covariance_oracle.py.
A float64 Cholesky inverse of S (condition 1e15) is itself off by 1e-6 .. 1e-4, and reordering its sums alone moves that error by up
to 2x: the margin of 8.  A wrong entry, index or sign shows at 1e-2 or more.

Measured on an MI355X (profiles/covariance.txt has the table, 24 rows): worst ratio e(device) / max e(float64 path) 1.03 (frames6,
initial states; every other row 0.11 .. 0.94), worst e(device) 2.3e-5 (full_td, solved states).  The kernel sums S, the Cholesky dot
products and the substitutions in twice the working precision, which is why it sits below the float64 path on most windows.

The exact properties are checked bit for bit: run to run, alone against inside a 300-window mixed batch against the reversed batch,
block (i, j) against block (j, i), the symmetry of diagonal blocks, and that a batch which computes covariances solves, fixes and
marginalises to the same bits as its twin that never does."""
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_cases as CC
import evaluate_cases as EC
import synth
import tcv_covariance as cv

pytestmark = pytest.mark.gpu

CASES = ("frames4", "frames6", "frames6_td", "full", "full_td", "constant_extrinsic", "relocalisation", "golden_prior", "landmarks200")
COMMON = [(("pose", -1), ("pose", -1)), (("pose", -1), ("sb", -1)), (("sb", -1), ("pose", -1)), (("pose", 0), ("pose", 0)), (("ex", 0), ("ex", 0)),
          (("pose", 1), ("pose", 1)), (("pose", 2), ("pose", 3))]


def hip(gpu, w, kw):
    """(tcv.Window, relocalisation pose or None) of a case"""
    W, relo = EC.hip_window(gpu, w, **kw)
    if relo is not None:
        W.set_relocalization(relo, 4, np.zeros(3), np.eye(3))
    return W, relo


def device_blocks(gpu, b, rq, window=0, **kw):
    cv.compute(b, rq, **kw)
    return [cv.block(b, window, k) for k in range(len(rq))], cv.status(b)


def gate(name, tag, ref, blocks, rq):
    e_dev = max(ref.e(C, bi, bj) for C, (bi, bj) in zip(blocks, rq))
    e_64 = max(ref.e_f64_block(bi, bj) for bi, bj in rq)
    print("covariance parity %-20s %-16s nc %3d e(device) %.2e e(float64 path) %.2e ratio %.2f" % (name, tag, ref.P.nc, e_dev, e_64, e_dev / e_64))
    assert e_dev <= 8 * e_64, (name, tag, e_dev, e_64)
    assert e_dev < 1e-3, (name, tag, e_dev)


def exact_properties(blocks, rq):
    at = {r: k for k, r in enumerate(rq)}
    for (bi, bj), k in at.items():
        if bi == bj:
            assert np.array_equal(blocks[k], blocks[k].T), (bi, "diagonal block not symmetric")
        elif (bj, bi) in at:
            assert np.array_equal(blocks[k], blocks[at[(bj, bi)]].T), (bi, bj, "block (i, j) is not block (j, i) transposed")


@pytest.mark.parametrize("name", CASES)
def test_parity_at_the_initial_and_at_the_solved_states(gpu, name):
    w, kw = CC.windows()[name]
    rq = CC.requests(name)
    W, relo = hip(gpu, w, kw)
    b = gpu.Batch([W])
    blocks, st = device_blocks(gpu, b, rq)
    assert st[0] == cv.OK
    ref = CC.reference(name)
    gate(name, "initial", ref, blocks, rq)
    exact_properties(blocks, rq)
    again, _ = device_blocks(gpu, b, rq)
    assert all(np.array_equal(a, c) for a, c in zip(blocks, again)), "run to run"
    if not kw.get("estimate_extrinsic", True):
        assert not np.any(blocks[5]) and not np.any(blocks[6]) and blocks[5].shape == (6, 6)      # a constant block: zeros, as Ceres
    # the bulk getter and the one-problem call return the same bits
    assert all(np.array_equal(cv.block_all(b, k)[0], blocks[k]) for k in (0, 1))
    one, st1 = cv.problem_covariance(W, rq[:2])
    assert st1 == cv.OK and np.array_equal(one[0], blocks[0]) and np.array_equal(one[1], blocks[1])
    # at the solved states
    b.solve(gpu.default_options(4, True)); b.synchronize(); b.download_states()
    x = EC.oracle_state(ref.P, W, relo)
    solved, st = device_blocks(gpu, b, rq, at_solution=True)
    assert st[0] == cv.OK
    gate(name, "solved", CC.reference(name, x, key="solved"), solved, rq)
    exact_properties(solved, rq)
    assert not np.array_equal(solved[0], blocks[0])


@pytest.mark.parametrize("name", ("frames6", "full", "golden_prior"))
def test_parity_without_the_loss_function(gpu, name):
    w, kw = CC.windows()[name]
    rq = CC.requests(name)
    W, relo = hip(gpu, w, kw)
    b = gpu.Batch([W])
    with_loss, _ = device_blocks(gpu, b, rq)
    blocks, st = device_blocks(gpu, b, rq, apply_loss_function=False)
    assert st[0] == cv.OK and not np.array_equal(with_loss[0], blocks[0])
    gate(name, "initial, no loss", CC.reference(name, loss=False), blocks, rq)
    b.solve(gpu.default_options(4, True)); b.synchronize(); b.download_states()
    x = EC.oracle_state(CC.reference(name).P, W, relo)
    blocks, st = device_blocks(gpu, b, rq, at_solution=True, apply_loss_function=False)
    gate(name, "solved, no loss", CC.reference(name, x, loss=False, key="solved"), blocks, rq)


def test_alone_inside_a_mixed_batch_and_reversed_same_bits_and_rank_deficient_neighbours(gpu):
    """300 windows of mixed shapes, three of them without a gauge (neither prior nor lines): those report status 1 and zero blocks, the
    call returns TCV_OK, and every other window has the bits of its solo run -- in the batch and in the reversed batch."""
    names = [n for n in CASES if n != "landmarks200"]
    wins = [CC.windows()[n] for n in names] + [(CC.no_gauge(s), {}) for s in CC.NO_GAUGE_SEEDS]
    solo = []
    for w, kw in wins:
        W, _ = hip(gpu, w, kw)
        blocks, st = device_blocks(gpu, gpu.Batch([W]), COMMON)
        solo.append((blocks, int(st[0])))
    for k in range(len(names), len(wins)):
        assert solo[k][1] == cv.RANK_DEFICIENT and not any(np.any(B) for B in solo[k][0])
    assert all(s == cv.OK for _, s in solo[:len(names)])
    pick = [(7 * i) % len(wins) for i in range(300)]
    keep = [hip(gpu, *wins[p]) for p in pick]
    for order in (list(range(300)), list(range(299, -1, -1))):
        b = gpu.Batch([keep[i][0] for i in order])
        cv.compute(b, COMMON)
        st = cv.status(b)
        allb = [cv.block_all(b, k) for k in range(len(COMMON))]
        for pos, i in enumerate(order):
            ref_blocks, ref_st = solo[pick[i]]
            assert st[pos] == ref_st, (pos, i)
            for k in range(len(COMMON)):
                assert np.array_equal(allb[k][pos], ref_blocks[k]), (pos, i, k)
                assert np.all(np.isfinite(allb[k][pos]))


def test_a_raised_rank_gate_turns_a_fine_window_into_status_1(gpu):
    """the option reaches the kernel: a gate 30x and more above the window's smallest relative pivot (2.5e-10; tests/test_covariance_cpu.py
    checks the margin) gives status 1 and zero blocks, the default gives status 0"""
    W, _ = hip(gpu, *CC.windows()["full"])
    b = gpu.Batch([W])
    blocks, st = device_blocks(gpu, b, COMMON, min_relative_pivot=1e-8)
    assert st[0] == cv.RANK_DEFICIENT and not any(np.any(B) for B in blocks)
    blocks, st = device_blocks(gpu, b, COMMON)
    assert st[0] == cv.OK and all(np.any(B) for B in blocks)


@pytest.mark.parametrize("setting", ("chain", "dense", "cooperative"))
def test_a_twin_batch_that_never_computes_a_covariance_ends_with_the_same_bits(gpu, setting):
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
                cv.compute(b, COMMON)
            b.solve(gpu.default_options(6, True, workgroups_per_window=0 if setting == "cooperative" else 1))
            if with_cov:
                cv.compute(b, COMMON, at_solution=True)
            b.gauge_fix()
            if with_cov:
                cv.compute(b, COMMON[:2], at_solution=True)
            b.marginalize()
            if with_cov:
                cv.compute(b, COMMON, at_solution=True)
                assert list(cv.status(b)) == [cv.OK, cv.OK]
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
    L = cv.lib()
    w, kw = CC.windows()["frames6_td"]
    Wtd, _ = hip(gpu, w, kw)
    W6, _ = hip(gpu, *CC.windows()["frames6"])
    b = gpu.Batch([Wtd, W6])
    arr, n = cv.blocks([("td", 0)])
    o = cv.default_options()
    assert L.tcv_batch_compute_covariance(b.h, o, arr, n, None) == gpu.TCV_ERR_INVALID and b"lacks a requested block" in L.tcv_last_error()      # window 1 has no td
    arr, n = cv.blocks([("pose", 6)])
    assert L.tcv_batch_compute_covariance(b.h, o, arr, n, None) == gpu.TCV_ERR_INVALID and b"out of range" in L.tcv_last_error()
    out = np.zeros(81)
    assert L.tcv_batch_get_covariance(b.h, 0, 0, cv.dptr(out), 81, None, None) == gpu.TCV_ERR_INVALID and b"no covariance has been computed" in L.tcv_last_error()
    arr, n = cv.blocks([("pose", -1)])
    o.at_solution = 1
    assert L.tcv_batch_compute_covariance(b.h, o, arr, n, None) == gpu.TCV_ERR_INVALID and b"has not been solved" in L.tcv_last_error()
    o.at_solution = 0
    gpu.check(L.tcv_batch_compute_covariance(b.h, o, arr, n, None))
    assert L.tcv_batch_get_covariance(b.h, 2, 0, cv.dptr(out), 81, None, None) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_get_covariance(b.h, 0, 1, cv.dptr(out), 81, None, None) == gpu.TCV_ERR_INVALID
    assert L.tcv_batch_get_covariance(b.h, 0, 0, cv.dptr(out), 35, None, None) == gpu.TCV_ERR_INVALID and b"too small" in L.tcv_last_error()
    assert not np.any(out)
    st = np.zeros(3, np.int32)
    assert L.tcv_batch_covariance_status(b.h, cv.iptr(st), 3) == gpu.TCV_ERR_INVALID


def test_covariance_buffers_go_back_with_the_batch(gpu):
    W = [gpu.Window(synth.window_at(synth.make_windows(5, 2), k)) for k in range(2)]
    live0 = gpu.device_memory_stats()[0]
    b = gpu.Batch(W)
    live1 = gpu.device_memory_stats()[0]
    cv.compute(b, COMMON); cv.block(b, 1, 0)
    assert gpu.device_memory_stats()[0] > live1
    cv.compute(b, COMMON[:3]); cv.status(b)      # a new request list replaces the result buffers
    gpu.lib().tcv_batch_destroy(b.h); b.h = None
    assert gpu.device_memory_stats()[0] == live0
    cv.problem_covariance(W[0], COMMON[:1])
    assert gpu.device_memory_stats()[0] == live0


def test_ceres_shim_covariance(gpu, tmp_path):
    """include/tcv_ceres_shim.hpp tcvshim::Covariance, compiled and run the way tests/test_gpu_evaluate.py runs the example"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.LIB_PATH)
    exe = os.path.join(tmp_path, "estimator_shim_classes")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "estimator_shim_classes.cpp"),
                           "-L" + libdir, "-ltcv_hip", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"covariance of the newest pose: sigma_p (\S+) (\S+) (\S+) sigma_theta (\S+) (\S+) (\S+); ambient 7 x 7 last row and column zero: (\d); symmetric: (\d)", r.stdout)
    assert m, r.stdout
    sig = np.array([float(v) for v in m.groups()[:6]])
    assert np.all(np.isfinite(sig)) and np.all(sig > 0) and m.group(7) == "1" and m.group(8) == "1", r.stdout
