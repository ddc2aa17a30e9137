"""GPU parity of the marginalisation (MarginalizationInfo::marginalize, marginalization_factor.cpp:174-299)
against the golden vectors and the C oracle.  A' is a small difference of ~1e14 terms, so ~1e-7 relative is the FP64
reproducibility floor between any two implementations (SURVEY.md Appendix B.2 measures 4.8e-7 for the same maths with the factors
accumulated in another order); the factors J0, r0 are only defined up to eigenvector sign / rotation, so parity is gated on J0'J0
and J0'r0.  Every gate sits about one order of magnitude above the value measured on the MI355X (tests/dev/marg_floor.py,
profiles/r02_marg_floor.txt; round 1 gated at 1e-5 ... 1e-3 across the board):
    at bit-identical states      A' 5e-8 ... 1.6e-7   b' 1e-13 ... 4e-13      J0'r0 vs b' 1.6e-6 (35 of 75 eigenvalues of A' are thresholded)
    after each side's own solve  A' 1.5e-7 ... 5.2e-7 b' 2e-9 ... 5e-8        J0'r0 1.8e-5
    chained solve on that prior  final cost 1.2e-5, poses 6.5e-7 (the 1e-7 of the prior seen through 8 dogleg iterations)"""
import ctypes as C

import numpy as np
import pytest

import orc
import synth
from util import fmt_families, fro, golden_windows, rel, rel_by_family, state_families

pytestmark = pytest.mark.gpu


def marg_batch(tcv, wins, solve=True):
    W = [tcv.Window(w) for w in wins]
    MW = [tcv.margin_old_window(w) for w in wins]
    M = [tcv.Window(mw, share=W[k]) for k, mw in enumerate(MW)]
    drops = [tcv.margin_old_drops(W[k], MW[k]) for k in range(len(wins))]
    b = tcv.Batch(W, M, drops)
    if solve:
        b.solve(tcv.default_options(8, True))
    b.marginalize()
    b.synchronize()
    return W, b


def test_golden_marginalisation_after_solve(gpu):
    pre, main, z = golden_windows()
    W, b = marg_batch(gpu, [pre])
    P = b.prior(0); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (int(z["marg_m"]), int(z["marg_n"]))
    assert d["sizes"] == [int(s) for s in z["marg_sizes"]] and d["idx"] == [int(i) for i in z["marg_idx"]]
    kinds = {0: "pose", 1: "sb", 2: "ex"}
    want = [(kinds[int(k)], int(i)) for k, i in zip(z["marg_block_kind"], z["marg_block_index"])]
    assert gpu.shifted_prior_blocks(P, W[0]) == want                 # addr_shift of estimator.cpp:2027-2039
    assert fro(As, z["marg_A_schur"]) < 5e-6 and fro(bs, z["marg_b_schur"]) < 5e-7      # measured 5.2e-7 / 4.7e-8 (each side linearises at its own solve's states)
    JtJ = d["J0"].T @ d["J0"]
    assert fro(JtJ, z["marg_J0"].T @ z["marg_J0"]) < 5e-6                                 # measured 5.1e-7
    assert fro(d["J0"].T @ d["r0"], z["marg_J0"].T @ z["marg_r0"]) < 6e-5                 # measured 1.8e-5 (gate = 3 x: r0 = S^-1/2 V' b' amplifies the eigenvectors' rounding)
    assert rel(np.concatenate(d["x0"]), z["marg_x0"]) < 1e-7          # linearisation point = solved states (preMarginalize :110-129); measured 7.5e-9
    # reference invariants (marginalization_factor.cpp:297-298) up to the eps = 1e-8 thresholded null space (35 of 75 eigenvalues)
    assert fro(JtJ, As) < 5e-7 and fro(d["J0"].T @ d["r0"], bs) < 5e-5                    # measured 3.7e-8 / 1.5e-5 (3 x)
    # thresholded factor is positive semi-definite and ordered like SelfAdjointEigenSolver (ascending)
    rn = np.linalg.norm(d["J0"], axis=1)
    assert np.all(np.diff(rn) >= -1e-9 * rn.max())


def test_standalone_marginalise_at_given_state_vs_oracle(gpu):
    """tcv_marginalize on host-resident states: both sides linearise at bit-identical states."""
    batch = synth.make_windows(900, 2, frame_shift=-1)
    for k in range(2):
        w = synth.window_at(batch, k)
        O = orc.Window(w); O.solve(8, True); st = O.states(); po, dbg = O.marginalize_old()
        w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
        mw = gpu.margin_old_window(w2)
        Wm = gpu.Window(mw)
        dr = gpu.margin_old_drops(Wm, mw)
        arr = (gpu._dp * len(dr))(*dr)
        h = C.c_void_p()
        gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
        P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
        assert (d["m"], d["n"]) == (po["m"], po["n"])
        assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-11          # measured 1.6e-7 / 1.9e-13 at bit-identical states
        assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 2e-6
        assert fro(d["J0"].T @ d["r0"], dbg["b_schur"]) < 2e-5                             # measured 1.8e-6
        assert rel(np.concatenate(d["x0"]), np.concatenate([np.atleast_1d(v) for v in po["x0"]])) == 0.0


def test_marginalisation_with_an_incoming_prior(gpu):
    """second window of a chain: the prior itself is one of the marginalised factors (estimator.cpp:1913-1931)."""
    pre, main, z = golden_windows()
    W, b = marg_batch(gpu, [main])
    P = b.prior(0); d = P.export(); As, bs = P.schur()
    O = orc.Window(main); O.solve(8, True); po, dbg = O.marginalize_old()
    assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 5e-8                # measured 1.5e-7 / 2.2e-9 (round 1 gated both at 1e-4)
    assert fro(d["J0"].T @ d["J0"], po["J0"].T @ po["J0"]) < 2e-6


def test_prior_round_trip_and_chained_solve(gpu):
    """the prior exported by the GPU marginalisation is importable (checkpoint) and drives the next solve to the
    same optimum as the oracle chain, within the reproducibility floor of the prior."""
    pre, main, z = golden_windows()
    W, b = marg_batch(gpu, [pre])
    P = b.prior(0); d = P.export()
    d["blocks"] = gpu.shifted_prior_blocks(P, W[0])
    P2 = gpu.Prior.from_dict(d)
    d2 = P2.export()
    assert np.array_equal(d2["J0"], d["J0"]) and np.array_equal(d2["r0"], d["r0"]) and d2["idx"] == d["idx"]
    w = dict(main); w["prior"] = d
    Wn = gpu.Window(w)
    bn = gpu.Batch([Wn]); bn.solve(gpu.default_options(8, True)); bn.synchronize(); bn.download_states()
    s = bn.summaries()[0]
    O = orc.Window(main); so = O.solve(8, True)
    # Two correct priors (HIP-made and oracle-made: A' 4.7e-7, J0'r0 1.7e-5 apart -- r0 = S^-1/2 V'b' amplifies the small retained
    # eigenvalues) are two slightly different cost functions, so the two chains are gated on what is well-posed, not on the end state of
    # eight dogleg iterations on an ill-conditioned window (round-4 review, item 5a; profiles/r05_chained_prior_invariants.txt):
    # (1) the first trust-region step from the same states: cost at the start, model-cost decrease, step norm (measured 2.5e-10 / 7.4e-8 / 5e-16);
    r = lambda a, c: abs(a - c) / abs(c)
    assert r(s.initial_cost, so.initial_cost) < 1e-8
    assert r(s.model_cost_change[1], so.model_cost_change[1]) < 1e-6 and r(s.step_norm[1], so.step_norm[1]) < 1e-9
    # (2) the same accept / reject and dogleg-case sequence through all eight iterations;
    n1 = so.num_iterations
    assert s.num_iterations == n1
    assert [s.step_ok[i] for i in range(1, n1)] == [so.step_ok[i] for i in range(1, n1)]
    assert [s.dogleg_case[i] for i in range(1, n1)] == [so.dogleg_case[i] for i in range(1, n1)]
    # (3) the end states by the north_star's trajectory criterion -- positions within 1 mm (measured 1.2 um) --, and the final cost within
    # the difference of the two priors' own linear terms (first order: d cost ~ dx' d(J0'r0); measured 2.0e-5 against 1.7e-5)
    jtr = fro(d["J0"].T @ d["r0"], main["prior"]["J0"].T @ main["prior"]["r0"])
    assert np.abs(Wn.pose[:, :3] - O.states()["pose"][:, :3]).max() < 1e-5
    assert r(s.final_cost, so.final_cost) < 2.0 * jtr + 1e-7, (r(s.final_cost, so.final_cost), jtr)
    assert rel(Wn.pose, O.states()["pose"]) < 1e-5 and rel(Wn.sb, O.states()["sb"]) < 2e-5          # (regression bound, not a parity criterion: measured 6.4e-7 / 1.6e-6)
    # ... and with the prior's floor taken out -- the oracle solves the window with the SAME (GPU-made) prior -- the two solves agree at the
    # level of every other solve parity test: identical accept / reject and dogleg sequences, north_star's 1e-6 with margin
    O2 = orc.Window(w); so2 = O2.solve(8, True)
    n2 = so2.num_iterations
    assert s.num_iterations == n2
    assert [s.step_ok[i] for i in range(1, n2)] == [so2.step_ok[i] for i in range(1, n2)]
    assert [s.dogleg_case[i] for i in range(1, n2)] == [so2.dogleg_case[i] for i in range(1, n2)]
    assert abs(s.final_cost - so2.final_cost) < 1e-7 * so2.final_cost
    assert rel(Wn.pose, O2.states()["pose"]) < 1e-7 and rel(Wn.sb, O2.states()["sb"]) < 1e-6
    byf = rel_by_family(state_families(Wn.states()), state_families(O2.states()))          # ... within every parameter family
    print("chained solve on the GPU-made prior, states per family:", fmt_families(byf))
    assert all(v < 1e-6 for v in byf.values()), byf


def test_margin_second_new_prior_only(gpu):
    """MARGIN_SECOND_NEW (estimator.cpp:2047-2113): only the old prior is marginalised, dropping para_Pose[WINDOW_SIZE-1]
    (m = 6); kept blocks keep their frame index (addr_shift :2084-2104)."""
    import np_oracle as NO
    pre, main, z = golden_windows()
    Oc = orc.Window(main); Oc.solve(8, True); st = Oc.states()
    w2 = dict(main, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
    prob = NO.Problem(w2)
    po, dbg = NO.marginalize_second_new(prob, prob.x0())
    mw = gpu.margin_second_new_window(w2)
    Wm = gpu.Window(mw)
    assert gpu.lib().tcv_problem_num_residual_blocks(Wm.h) == 1
    dr = gpu.margin_second_new_drops(Wm)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (6, po["n"]) == (6, main["prior"]["n"] - 6)
    assert d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("MARGIN_SECOND_NEW: A' %.2e b' %.2e J0'J0 %.2e J0'r0 %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"]), fro(d["J0"].T @ d["J0"], po["J0"].T @ po["J0"]),
                                                                    fro(d["J0"].T @ d["r0"], po["J0"].T @ po["r0"])))
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8
    assert fro(d["J0"].T @ d["J0"], po["J0"].T @ po["J0"]) < 2e-6
    assert fro(d["J0"].T @ d["r0"], po["J0"].T @ po["r0"]) < 1e-10      # measured 1.8e-13 (MARGIN_SECOND_NEW of a full-rank prior: no thresholded noise directions)
    assert rel(np.concatenate(d["x0"]), np.concatenate([np.atleast_1d(v) for v in po["x0"]])) == 0.0
    # kept blocks: every prior block except pose WINDOW_SIZE-1, un-shifted
    W = main["pose"].shape[0] - 1
    assert po["blocks"] == [b for b in main["prior"]["blocks"] if tuple(b) != ("pose", W - 1)]
    base = {"pose": (Wm.pose.ctypes.data, 56), "sb": (Wm.sb.ctypes.data, 72), "ex": (Wm.ex.ctypes.data, 56)}
    addrs = (gpu._dp * len(d["sizes"]))()
    gpu.check(gpu.lib().tcv_prior_keep_block_addresses(P.h, addrs))
    got = []
    for a in addrs:
        a = C.cast(a, C.c_void_p).value
        for nm, (b0, stride) in base.items():
            if b0 <= a < b0 + stride * (11 if nm != "ex" else 1):
                got.append((nm, (a - b0) // stride))
    assert got == [tuple(b) for b in po["blocks"]]


def test_margin_second_new_with_a_prior_that_does_not_fit_the_lds(gpu):
    """The prior phase stages J0 in the region of the packed A when its stored rows fit there and forms J0'J0 on the matrix cores; otherwise
    it reads J0 from HBM, entry by entry.  MARGIN_SECOND_NEW has the small region (pos = 75), and a prior without zero rows (the golden
    prior's 34 zero rows given a unit entry each: 75 x 75 > 70 x 71 stored entries) does not fit: the same gates as
    test_margin_second_new_prior_only, at the window's own state."""
    import np_oracle as NO
    pre, main, z = golden_windows()
    J0 = np.array(main["prior"]["J0"], copy=True)
    zero = np.flatnonzero(~J0.any(axis=1))
    J0[zero, zero] = 1.0
    main = dict(main, prior=dict(main["prior"], J0=J0))
    prob = NO.Problem(main)
    po, dbg = NO.marginalize_second_new(prob, prob.x0())
    mw = gpu.margin_second_new_window(main)
    Wm = gpu.Window(mw)
    dr = gpu.margin_second_new_drops(Wm)
    H = gpu.marg_plan(Wm, dr)[0]
    ne = H.n + (H.n & 1)
    assert H.prior_k0 == 0 and H.prior_n * H.prior_n > max(H.pos * (H.pos + 1) // 2, ne * (ne + 1))      # (csrc/tcv_marg.hip marg_prior: in_lds is false)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (6, po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("MARGIN_SECOND_NEW, prior from HBM: A' %.2e b' %.2e J0'J0 %.2e J0'r0 %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"]),
          fro(d["J0"].T @ d["J0"], po["J0"].T @ po["J0"]), fro(d["J0"].T @ d["r0"], po["J0"].T @ po["r0"])))
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8
    assert fro(d["J0"].T @ d["J0"], po["J0"].T @ po["J0"]) < 2e-6
    assert fro(d["J0"].T @ d["r0"], po["J0"].T @ po["r0"]) < 1e-10


def test_large_drop_set_uses_landmark_pivots(gpu):
    """a 150-feature front end anchors far more landmarks in the oldest frame than the LDS-resident eigen-solver takes
    (m <= 64): the marginalised inverse depths are then eliminated by scalar pivots and only the frame part (15) goes through
    the eigen pseudo-inverse.  Same A', b' as the reference's one-piece eigen-decomposition of A_mm (oracle) within the
    reproducibility floor; m keeps the reference's meaning (all marginalised dims)."""
    batch = synth.make_windows(902, 1, n_landmarks=400, frame_shift=-1)
    w = synth.window_at(batch, 0)
    O = orc.Window(w); O.solve(4, True); st = O.states(); po, dbg = O.marginalize_old()
    assert po["m"] > 64
    w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
    mw = gpu.margin_old_window(w2)
    Wm = gpu.Window(mw)
    dr = gpu.margin_old_drops(Wm, mw)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("block mode (m = %d): A' %.2e b' %.2e" % (po["m"], fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"])))
    assert fro(As, dbg["A_schur"]) < 1e-5 and fro(bs, dbg["b_schur"]) < 1e-5
    assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 1e-5
    assert rel(np.concatenate(d["x0"]), np.concatenate([np.atleast_1d(v) for v in po["x0"]])) == 0.0


BLOCK_PATHS = {      # name -> (frames kept, switch, what the packed plan must say: chunked?, C behind the staging records?)
    "scalar_pivots": (11, "TCV_MARG_BLOCK_SERIAL", (False, False)),
    "c_behind_the_records": (6, None, (True, True)),
}


@pytest.mark.parametrize("name", list(BLOCK_PATHS))
def test_block_mode_paths_of_the_projection_phase_vs_oracle(gpu, monkeypatch, name):
    """Block mode (more than 64 dropped dims: 344 landmarks anchor 50 in frame 0) on the paths of the projection phase that
    test_large_drop_set_uses_landmark_pivots does not take: factor by factor with a scalar pivot per landmark (TCV_MARG_BLOCK_SERIAL), and the
    chunked path with the couplings C behind the staging records (a window of 6 frames: n = 45 leaves no room in the region of the packed
    A).  The plan says which path it is; A', b' against the C oracle at the same state, with the gates of
    test_large_drop_set_uses_landmark_pivots.  Measured: scalar pivots 2.5e-7 / 1.2e-12, C behind the records 9.1e-8 / 2.9e-12.
    (Block mode with ProjectionTdFactors takes the scalar pivots too, but has no reference good to these gates: the C oracle has no Td,
    and the NumPy oracle's one-piece pseudo-inverse of this 65-dim A_mm is 7.9e-4 / 1.4e-3 from the C oracle's on the window without Td.)"""
    from util import sub_window
    frames, switch, (chunked, c_in_r2) = BLOCK_PATHS[name]
    w = synth.window_at(synth.make_windows(902, 1, n_landmarks=344, frame_shift=-1), 0)
    if frames < 11:
        w = sub_window(w, frames)
    po, dbg = orc.Window(w).marginalize_old()
    assert po["m"] > 64
    if switch:
        monkeypatch.setenv(switch, "1")
    mw = gpu.margin_old_window(w)
    Wm = gpu.Window(mw)
    dr = gpu.margin_old_drops(Wm, mw)
    H = gpu.marg_plan(Wm, dr)[0]
    r1 = max(H.pos * (H.pos + 1) // 2, (H.n + (H.n & 1)) * (H.n + (H.n & 1) + 1))      # doubles of the region of the packed A (csrc/tcv_marg.hip marg_carve)
    assert H.block_mode == 1 and (H.cb_off >= 0, H.cb_off >= r1) == (chunked, c_in_r2)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("block mode, %s (m = %d, n = %d): A' %.2e b' %.2e" % (name, po["m"], po["n"], fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"])))
    assert fro(As, dbg["A_schur"]) < 1e-5 and fro(bs, dbg["b_schur"]) < 1e-5
    assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 1e-5


@pytest.mark.parametrize("nt", ["256", "512"])
def test_both_launch_shapes_of_the_marginalisation_kernel(gpu, monkeypatch, nt):
    """The kernel runs as one 512-thread workgroup per CU or, for batches larger than the CU count whose windows fit 80 KB of LDS, as
    two 256-thread workgroups per CU (csrc/tcv_marg_host.cpp marg_launch_shape; chosen by batch size, forced here through TCV_MARG_NT).  The accumulation of
    A and the Schur complement do not depend on the shape: A', b' bit for bit; the eigen step differs in rounding only (4-section vs
    7-section eigenvalue search, three vs four lanes per column in the back-transformation): J0'J0 = A' and J0'r0 = b' to the same floor."""
    pre, main, z = golden_windows()
    more = synth.make_windows(910, 3, frame_shift=-1)
    wins = [pre, main] + [synth.window_at(more, k) for k in range(3)]
    monkeypatch.setenv("TCV_MARG_NT", nt)
    W, b = marg_batch(gpu, wins)
    assert list(b.marg_status()) == [0] * len(wins)
    monkeypatch.setenv("TCV_MARG_NT", "512")
    W2, b2 = marg_batch(gpu, wins)
    for k in range(len(wins)):
        P = b.prior(k); d = P.export(); As, bs = P.schur()
        As2, bs2 = b2.prior(k).schur(); d2 = b2.prior(k).export()
        assert np.array_equal(As, As2) and np.array_equal(bs, bs2)
        # measured (both shapes alike: the defect is the thresholded noise eigenvalue, -4e-2 against |A'| = 3e5): 1.3e-7 / 1.4e-5
        assert fro(d["J0"].T @ d["J0"], As) < 2e-6 and fro(d["J0"].T @ d["r0"], bs) < 5e-5
        assert fro(d["J0"].T @ d["J0"], d2["J0"].T @ d2["J0"]) < 1e-9


def test_shortcuts_of_the_marginalisation_are_bit_identical_to_the_plain_paths(gpu, monkeypatch):
    """Three shortcuts of the batch marginalisation reuse what the batch already has: the IMU factor's sqrt_info from the solve kernel
    (TCV_MARG_OWN_SQRT=1: factorise the covariance again), the prior's J0 | r0 | x0 from the solve batch's data pool (TCV_MARG_OWN_PRIOR=1:
    an own copy), and the per-entry accumulation of the point factors (TCV_MARG_PROJ_SERIAL=1: factor by factor with a barrier each).
    Each must leave every bit of the result alone."""
    pre, main, z = golden_windows()
    more = synth.make_windows(920, 2, frame_shift=-1)
    wins = [pre, main, synth.window_at(more, 0), synth.window_at(more, 1)]

    def run():
        W, b = marg_batch(gpu, wins)
        return [(b.prior(k).export(), b.prior(k).schur()) for k in range(len(wins))]

    ref = run()
    for var in ("TCV_MARG_OWN_SQRT", "TCV_MARG_OWN_PRIOR", "TCV_MARG_PROJ_SERIAL"):
        monkeypatch.setenv(var, "1")
        got = run()
        monkeypatch.delenv(var)
        for (d0, (A0, b0)), (d1, (A1, b1)) in zip(ref, got):
            assert np.array_equal(A0, A1) and np.array_equal(b0, b1), var
            assert np.array_equal(d0["J0"], d1["J0"]) and np.array_equal(d0["r0"], d1["r0"]), var


def test_round3_eigen_solver_against_round2_paths(gpu, monkeypatch):
    """Round 3 locates only the eigenvalues of A' above eps (they are the only ones marginalization_factor.cpp:284-293 keeps) and applies the
    reflectors in blocks on the matrix cores.  TCV_MARG_EIG_FLAGS brings round 2's paths back (1: every eigenvalue by 4-section, 2: reflector
    by reflector on the VALU): A' and b' are formed before the eigen-solver and must not move a bit; the factors agree as far as an
    eigen-decomposition of A' is defined -- J0'J0, J0'r0, the number of thresholded rows -- to the accuracy of the solver (1e-9 of |A'|)."""
    pre, main, z = golden_windows()
    more = synth.make_windows(930, 3, frame_shift=-1)
    wins = [pre, main] + [synth.window_at(more, k) for k in range(3)]

    def run():
        W, b = marg_batch(gpu, wins)
        assert not b.marg_status().any()                 # nobody on the Jacobi safety net
        return [(b.prior(k).export(), b.prior(k).schur()) for k in range(len(wins))]

    ref = run()
    for d, (A, bb) in ref:
        zero = ~d["J0"].any(axis=1)
        assert zero.sum() >= 4 and not zero[zero.sum():].any()      # the thresholded rows (at least the gauge) lead, ascending eigenvalues follow
    for flags in ("1", "2", "3"):
        monkeypatch.setenv("TCV_MARG_EIG_FLAGS", flags)
        got = run()
        monkeypatch.delenv("TCV_MARG_EIG_FLAGS")
        for (d0, (A0, b0)), (d1, (A1, b1)) in zip(ref, got):
            assert np.array_equal(A0, A1) and np.array_equal(b0, b1), flags
            assert (~d0["J0"].any(axis=1)).sum() == (~d1["J0"].any(axis=1)).sum(), flags
            assert fro(d0["J0"].T @ d0["J0"], d1["J0"].T @ d1["J0"]) < 1e-9, flags
            assert np.linalg.norm(d0["J0"].T @ d0["r0"] - d1["J0"].T @ d1["r0"]) <= 1e-7 * np.linalg.norm(b0), flags


def test_prior_without_its_zero_rows_is_bit_identical(gpu, monkeypatch):
    """The rows of J0 | r0 that the marginalisation thresholded are exact zeros; the packer drops them (WinHdr::prior_k0) and the solve and the
    marginalisation work on the stored rows with the accumulation chains of the full matrix.  TCV_PRIOR_FULL=1 packs every row: states, costs,
    traces and the next prior must agree to the bit, with a third less window data."""
    pre, main, z = golden_windows()

    def run():
        W, b = marg_batch(gpu, [main])
        b.download_states()
        s = b.summaries()[0]
        P = b.prior(0)
        return (W[0].pose.copy(), W[0].sb.copy(), [s.cost[i] for i in range(s.num_iterations)], s.final_cost, P.export(), P.schur(), W[0].plan_stats()["window_doubles"])

    ref = run()
    monkeypatch.setenv("TCV_PRIOR_FULL", "1")
    full = run()
    monkeypatch.delenv("TCV_PRIOR_FULL")
    assert np.array_equal(ref[0], full[0]) and np.array_equal(ref[1], full[1])
    assert ref[2] == full[2] and ref[3] == full[3]
    assert np.array_equal(ref[4]["J0"], full[4]["J0"]) and np.array_equal(ref[4]["r0"], full[4]["r0"])
    assert np.array_equal(ref[5][0], full[5][0]) and np.array_equal(ref[5][1], full[5][1])
    n = z["marg_J0"].shape[0]
    k0 = int((~z["marg_J0"].any(axis=1)).sum())
    assert full[6] - ref[6] == k0 * n + k0 and k0 > 10


def _standalone(gpu, w2):
    mw = gpu.margin_old_window(w2)
    Wm = gpu.Window(mw)
    dr = gpu.margin_old_drops(Wm, mw)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    return gpu.Prior(h)


def test_dropped_block_through_cholesky_or_eigen_decomposition(gpu, monkeypatch):
    """Amm^+ (marginalization_factor.cpp:267-272).  When 1 / trace(Amm^-1) > eps proves every eigenvalue above eps, the kernel forms
    Arm Amm^-1 Amr from the Cholesky factor; TCV_MARG_EIG_MM=1 forces the reference's eigen-decomposition for every window.  Both against
    the oracle (eigen-decomposition) at identical states, and against each other."""
    batch = synth.make_windows(900, 2, frame_shift=-1)
    for k in range(2):
        w = synth.window_at(batch, k)
        O = orc.Window(w); O.solve(8, True); st = O.states(); po, dbg = O.marginalize_old()
        w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
        res = {}
        for mode in ("chol", "eig"):
            if mode == "eig":
                monkeypatch.setenv("TCV_MARG_EIG_MM", "1")
            else:
                monkeypatch.delenv("TCV_MARG_EIG_MM", raising=False)
            P = _standalone(gpu, w2); d = P.export(); As, bs = P.schur()
            res[mode] = (As, bs, d)
            assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-11
            assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 2e-6 and fro(d["J0"].T @ d["r0"], dbg["b_schur"]) < 2e-5
        print("cholesky vs eigen: A' %.2e b' %.2e" % (fro(res["chol"][0], res["eig"][0]), fro(res["chol"][1], res["eig"][1])))
        assert fro(res["chol"][0], res["eig"][0]) < 2e-6 and fro(res["chol"][1], res["eig"][1]) < 1e-11
        assert not np.array_equal(res["chol"][0], res["eig"][0])      # the two paths are really different code


def test_rank_deficient_dropped_block_takes_the_eigen_path(gpu):
    """A landmark seen without parallax (its only other observation from a frame with the anchor frame's pose) has a zero row in Amm:
    the rank proof of the Cholesky path fails and the pseudo-inverse drops that eigenvalue, as the reference does (:267-272)."""
    batch = synth.make_windows(905, 1, frame_shift=-1)
    w = synth.window_at(batch, 0)
    pr = w["proj"]
    fi, fj, lm = np.asarray(pr["frame_i"]), np.asarray(pr["frame_j"]), np.asarray(pr["landmark"])
    l0 = int(lm[(fi == 0) & (fj == 1)][0])
    keep = ~((lm == l0) & ~((fi == 0) & (fj == 1)))
    w = dict(w, proj={k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (len(fi),) else v) for k, v in pr.items()})
    pose = np.array(w["pose"], copy=True); pose[1] = pose[0]
    w = dict(w, pose=pose)
    po, dbg = orc.Window(w).marginalize_old()
    P = _standalone(gpu, w); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (po["m"], po["n"])
    print("rank-deficient Amm: A' %.2e b' %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"])))
    assert fro(As, dbg["A_schur"]) < 1e-5 and fro(bs, dbg["b_schur"]) < 1e-5
    assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 1e-5


def test_marginalise_error_paths(gpu):
    batch = synth.make_windows(901, 1)
    w = synth.window_at(batch, 0)
    W = gpu.Window(w)
    h = C.c_void_p()
    bogus = np.zeros(7)
    arr = (gpu._dp * 1)(gpu.dptr(bogus))
    assert gpu.lib().tcv_marginalize(W.h, arr, 1, C.byref(h)) in (gpu.TCV_ERR_INVALID, gpu.TCV_ERR_UNSUPPORTED)


def test_marginalisation_of_replay_windows_one_by_one_vs_oracle(gpu):
    """MARGIN_OLD of every keyframe window of a replay (different numbers of landmarks anchored in the oldest frame => different m,
    incoming priors from the chain) at identical, gauge-fixed states: (m, n), kept blocks, A' and b' against the C oracle."""
    import np_oracle as NO
    import replay
    from replay_oracle import OracleBackend

    got = []

    class Spy(OracleBackend):
        def optimize(self, win, flag, ni, fi):
            out = super().optimize(win, flag, ni, fi)
            if flag == replay.MARGIN_OLD:
                got.append(dict(win, pose=out["pose"], speedbias=out["sb"], ex_pose=out["ex"], lam=out["lam"]))
            return out

    stream = replay.simulate_stream_euroc("V1_02_medium", 36, start_s=5.0, max_features=50, max_lines=0)
    replay.run(stream, Spy(), num_iterations=8)
    assert len(got) >= 15
    ms = set()
    worstA = worstb = 0.0
    for w2 in got:
        po, dbg = orc.Window(w2).marginalize_old()
        mw = gpu.margin_old_window(w2)
        Wm = gpu.Window(mw)
        dr = gpu.margin_old_drops(Wm, mw)
        arr = (gpu._dp * len(dr))(*dr)
        h = C.c_void_p()
        gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
        P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
        assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == list(po["sizes"])
        ms.add(d["m"])
        worstA = max(worstA, fro(As, dbg["A_schur"])); worstb = max(worstb, fro(bs, dbg["b_schur"]))
        assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 1e-5
    print("m values", sorted(ms), "worst A' %.2e b' %.2e" % (worstA, worstb))
    assert len(ms) >= 4 and worstA < 5e-6 and worstb < 1e-8


def test_marginalisation_keeps_a_constant_extrinsic(gpu):
    """ESTIMATE_EXTRINSIC = 0 (what euroc_config.yaml ships): para_Ex_Pose is SetParameterBlockConstant in the solve
    (estimator.cpp:1694-1698) but MarginalizationInfo knows nothing about constness -- the block stays in keep_block_size / idx / data
    and its Jacobian columns are accumulated (marginalization_factor.cpp:89-108, :176-194): n = 75, not 69.  MARGIN_OLD and
    MARGIN_SECOND_NEW against the oracles at bit-identical states, and the chained solve with the extrinsic held constant."""
    import np_oracle as NO
    pre, main, z = golden_windows()
    for w, want_n in ((pre, None), (main, 75)):
        O = orc.Window(w, ex_constant=True); O.solve(8, True); st = O.states(); po, dbg = O.marginalize_old()
        assert np.array_equal(st["ex"], w["ex_pose"])                      # constant in the solve
        w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
        mw = gpu.margin_old_window(w2)
        Wm = gpu.Window(mw, estimate_extrinsic=False)
        dr = gpu.margin_old_drops(Wm, mw)
        arr = (gpu._dp * len(dr))(*dr)
        h = C.c_void_p()
        gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
        P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
        assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == list(po["sizes"]) and d["idx"] == list(po["idx"])
        assert d["sizes"][-1] == 7 and ("ex", 0) in gpu.shifted_prior_blocks(P, Wm)
        if want_n:
            assert d["n"] == want_n
        print("constant extrinsic MARGIN_OLD: A' %.2e b' %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"])))
        assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8
        assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 2e-6
    # the solve with the extrinsic constant and a prior that holds it (columns of J0 without a tangent index)
    Wn = gpu.Window(main, estimate_extrinsic=False)
    bn = gpu.Batch([Wn]); bn.solve(gpu.default_options(8, True)); bn.synchronize(); bn.download_states()
    s = bn.summaries()[0]
    O = orc.Window(main, ex_constant=True); so = O.solve(8, True)
    assert [s.step_ok[i] for i in range(9)] == [so.step_ok[i] for i in range(9)]
    assert abs(s.final_cost - so.final_cost) < 1e-6 * so.final_cost
    assert rel(Wn.pose, O.states()["pose"]) < 1e-6 and np.array_equal(Wn.ex, main["ex_pose"])
    # MARGIN_SECOND_NEW: the old prior alone, pose WINDOW_SIZE - 1 dropped, the constant extrinsic kept
    st = O.states()
    w2 = dict(main, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
    prob = NO.Problem(w2, ex_constant=True)
    po, dbg = NO.marginalize_second_new(prob, prob.x0())
    mw = gpu.margin_second_new_window(w2)
    Wm = gpu.Window(mw, estimate_extrinsic=False)
    dr = gpu.margin_second_new_drops(Wm)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (6, po["n"]) == (6, main["prior"]["n"] - 6) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8


def test_batch_with_windows_that_are_only_solved(gpu):
    """tcv_batch_create: single entries of marg_problems may be NULL -- the windows of a lock-step frame form ONE batch whether or not they
    marginalise (a MARGIN_SECOND_NEW frame whose prior does not hold para_Pose[WINDOW_SIZE - 1] only solves, estimator.cpp:2049-2050).
    The marginalised windows give the bits of an all-marginalising batch, the others have no prior."""
    tcv = gpu
    B = 5
    wins = [synth.window_at(synth.make_windows(7300, B), k) for k in range(B)]

    def run(skip):
        W = [tcv.Window(w) for w in wins]
        MW = [tcv.margin_old_window(w) for w in wins]
        M = [None if k in skip else tcv.Window(MW[k], share=W[k]) for k in range(B)]
        drops = [None if k in skip else tcv.margin_old_drops(W[k], MW[k]) for k in range(B)]
        b = tcv.Batch(W, M, drops)
        b.solve(tcv.default_options(8, True)); b.gauge_fix(); b.marginalize(); b.synchronize(); b.download_states(); b.download_priors()
        return W, b, b.summaries()

    W0, b0, s0 = run(set())
    W1, b1, s1 = run({1, 3})
    assert list(b1.marg_status()) == [0] * B
    pd = b1.priors_device(); ph = b1.priors()
    for k in range(B):
        assert s0[k].final_cost == s1[k].final_cost and np.array_equal(W0[k].pose, W1[k].pose) and np.array_equal(W0[k].lam, W1[k].lam)
        if k in (1, 3):
            assert pd[k] is None and ph[k] is None
            with pytest.raises(tcv.TcvError):
                b1.prior(k)
        else:
            e0, e1, ed = b0.prior(k).export(), b1.prior(k).export(), pd[k].export()
            for key in ("J0", "r0"):
                assert np.array_equal(e0[key], e1[key]) and np.array_equal(e0[key], ed[key]), (k, key)


def test_marginalisation_problems_attached_while_the_solve_runs_give_the_same_priors(gpu):
    """tcv_batch_attach_marginalization: a batch created without marginalisation problems takes them after its solve has been launched (their
    packing and upload overlap the solve; the marginalisation then forms the IMU factor's sqrt_info itself instead of taking the solve's
    export) -- states and priors bit for bit those of the batch that was created with them"""
    tcv = gpu
    B = 6
    batch = synth.make_windows(9500, B)
    wins = [synth.window_at(batch, k) for k in range(B)]
    opts = tcv.default_options(8, True)

    def run(attach_late):
        W = [tcv.Window(w) for w in wins]
        MW = [tcv.margin_old_window(w) for w in wins]
        M = [tcv.Window(MW[k], share=W[k]) for k in range(B)]
        drops = [tcv.margin_old_drops(W[k], MW[k]) for k in range(B)]
        if attach_late:
            b = tcv.Batch(W)
            b.solve(opts); b.gauge_fix()
            b.attach_marginalization(M, drops)
            with pytest.raises(tcv.TcvError):
                b.attach_marginalization(M, drops)      # once per batch
        else:
            b = tcv.Batch(W, M, drops)
            b.solve(opts); b.gauge_fix()
        b.marginalize(); b.synchronize(); b.download_states()
        assert list(b.marg_status()) == [0] * B
        b.download_priors(compact=True)
        return [w.states() for w in W], [p.export() for p in b.priors()]

    x0, p0 = run(False)
    x1, p1 = run(True)
    for k in range(B):
        for key in ("pose", "sb", "ex", "lam"):
            assert np.array_equal(x0[k][key], x1[k][key]), (k, key)
        assert np.array_equal(p0[k]["J0"], p1[k]["J0"]) and np.array_equal(p0[k]["r0"], p1[k]["r0"])
        assert all(np.array_equal(a, c) for a, c in zip(p0[k]["x0"], p1[k]["x0"]))


def test_margin_old_without_the_long_imu_factor(gpu):
    """estimator.cpp:1933: the IMU factor (0, 1) joins the marginalisation only `if (pre_integrations[1]->sum_dt < 10.0)`.  A window whose first
    interval is longer marginalises frame 0 from the prior and the point factors anchored there alone: same layout (m = 15 + landmarks of frame
    0, kept blocks), same A', b' as the oracle at bit-identical states."""
    pre, main, z = golden_windows()
    im = dict(main["imu"]); sd = np.array(im["sum_dt"], dtype=float).copy(); sd[0] = 11.0; im["sum_dt"] = sd
    w = dict(main, imu=im)
    O = orc.Window(w); O.solve(8, True); st = O.states(); po, dbg = O.marginalize_old()
    w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
    mw = gpu.margin_old_window(w2)
    assert len(mw["imu"]["frame_i"]) == 0
    Wm = gpu.Window(mw)
    dr = gpu.margin_old_drops(Wm, mw)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (po["m"], po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("MARGIN_OLD without the IMU factor: A' %.2e b' %.2e J0'J0 %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"]), fro(d["J0"].T @ d["J0"], dbg["A_schur"])))
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8
    assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 2e-6
    # ... and in a batch behind its own solve (the solve drops the factor from the chain, the marginalisation from its factor set)
    W, b = marg_batch(gpu, [w])
    P2 = b.prior(0); d2 = P2.export(); As2, bs2 = P2.schur()
    assert (d2["m"], d2["n"]) == (po["m"], po["n"])
    assert fro(As2, dbg["A_schur"]) < 5e-6 and fro(bs2, dbg["b_schur"]) < 5e-7


def test_margin_old_with_no_landmark_anchored_in_the_oldest_frame(gpu):
    """m = 15: every feature of the window started after frame 0, so MARGIN_OLD drops para_Pose[0] and para_SpeedBias[0] alone
    (the prior and the IMU factor are the only residual blocks MarginalizationInfo receives, estimator.cpp:1913-1947)"""
    pre, main, z = golden_windows()
    pr = {k: np.asarray(v) for k, v in main["proj"].items()}
    keep = pr["frame_i"] != 0
    # landmarks are renumbered in order of first appearance among the kept factors
    order, remap = [], {}
    for l in pr["landmark"][keep]:
        if int(l) not in remap:
            remap[int(l)] = len(order); order.append(int(l))
    proj = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == keep.shape else v) for k, v in pr.items()}
    proj["landmark"] = np.array([remap[int(l)] for l in proj["landmark"]], dtype=np.int64)
    w = dict(main, proj=proj, lam=np.asarray(main["lam"])[order])
    O = orc.Window(w); O.solve(8, True); st = O.states(); po, dbg = O.marginalize_old()
    assert po["m"] == 15
    w2 = dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
    mw = gpu.margin_old_window(w2)
    assert len(mw["proj"]["frame_i"]) == 0 and len(mw["imu"]["frame_i"]) == 1
    Wm = gpu.Window(mw)
    dr = gpu.margin_old_drops(Wm, mw)
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(gpu.lib().tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h); d = P.export(); As, bs = P.schur()
    assert (d["m"], d["n"]) == (15, po["n"]) and d["sizes"] == po["sizes"] and d["idx"] == po["idx"]
    print("MARGIN_OLD, m = 15: A' %.2e b' %.2e" % (fro(As, dbg["A_schur"]), fro(bs, dbg["b_schur"])))
    assert fro(As, dbg["A_schur"]) < 2e-6 and fro(bs, dbg["b_schur"]) < 1e-8
    assert fro(d["J0"].T @ d["J0"], dbg["A_schur"]) < 2e-6
    W, b = marg_batch(gpu, [w])
    As2, bs2 = b.prior(0).schur()
    assert b.prior(0).dims()[:2] == (15, po["n"]) and fro(As2, dbg["A_schur"]) < 5e-6 and fro(bs2, dbg["b_schur"]) < 5e-7


def test_marginalisation_that_keeps_nothing_returns_the_references_empty_prior(gpu):
    """Every block the factors touch is dropped: the reference's marginalize() runs with n = pos - m = 0 (marginalization_factor.cpp:174-194)
    and the estimator carries the empty MarginalizationInfo into the next frame, where its factor has no residuals over no blocks
    (estimator.cpp:2040-2043, :1714-1720).  Found by fuzz seed 1306 (frame 0 seen by line factors alone, its IMU factor left out); here: the
    IMU factor (0, 1) alone, all four of its blocks dropped -- standalone, inside a batch next to ordinary windows, and the solve on it."""
    L = gpu.lib()
    w = {k: v for k, v in synth.window_at(synth.make_windows(905, 1), 0).items() if k != "prior"}
    mw = gpu.margin_old_window(w)
    none = np.zeros(0, int)
    npj = len(mw["proj"]["frame_i"])
    mw["proj"] = {k: (np.asarray(v)[none] if isinstance(v, np.ndarray) and v.shape[:1] == (npj,) else v) for k, v in mw["proj"].items()}
    Wm = gpu.Window(mw)
    dr = [Wm.block_ptr("pose", 0), Wm.block_ptr("sb", 0), Wm.block_ptr("pose", 1), Wm.block_ptr("sb", 1)]
    arr = (gpu._dp * len(dr))(*dr)
    h = C.c_void_p()
    gpu.check(L.tcv_marginalize(Wm.h, arr, len(dr), C.byref(h)))
    P = gpu.Prior(h)
    assert P.dims() == (30, 0, 0, 0)                      # m = 6 + 9 + 6 + 9 dropped tangent dims, nothing kept
    d = P.export()
    assert d["sizes"] == [] and d["J0"].shape == (0, 0) and d["r0"].shape == (0,)
    # the next frame's problem takes it as a factor without residuals: same solve as without a prior
    W0 = gpu.Window(w); n_res0 = L.tcv_problem_num_residual_blocks(W0.h)
    W1 = gpu.Window(w, prior=P)
    assert L.tcv_problem_num_residual_blocks(W1.h) == n_res0
    b = gpu.Batch([W0, W1]); b.solve(gpu.default_options(8, True)); b.synchronize(); b.download_states()
    s = b.summaries()
    assert s[0].final_cost == s[1].final_cost and np.array_equal(W0.pose, W1.pose)
    # inside a batch: window 0 marginalises as usual, window 1 keeps nothing
    w_ok = synth.window_at(synth.make_windows(906, 1, frame_shift=-1), 0)
    Wk = gpu.Window(w_ok); mk = gpu.margin_old_window(w_ok); Mk = gpu.Window(mk, share=Wk)
    We = gpu.Window(w); Me = gpu.Window(mw, share=We)
    dre = [Me.block_ptr("pose", 0), Me.block_ptr("sb", 0), Me.block_ptr("pose", 1), Me.block_ptr("sb", 1)]
    b2 = gpu.Batch([Wk, We], [Mk, Me], [gpu.margin_old_drops(Wk, mk), dre])
    b2.solve(gpu.default_options(8, True)); b2.marginalize(); b2.synchronize()
    st = np.zeros(2, np.int32)
    gpu.check(L.tcv_batch_marg_status(b2.h, gpu.iptr(st), 2))
    assert list(st) == [0, 0]
    p0, p1 = b2.prior(0), b2.prior(1)
    assert p0.dims()[1] > 0 and p1.dims() == (30, 0, 0, 0)
    Wr = gpu.Window(w_ok); Mr = gpu.Window(mk, share=Wr)
    b3 = gpu.Batch([Wr], [Mr], [gpu.margin_old_drops(Wr, mk)])
    b3.solve(gpu.default_options(8, True)); b3.marginalize(); b3.synchronize()
    assert np.array_equal(p0.export()["J0"], b3.prior(0).export()["J0"])      # the empty neighbour changes nothing for the others
    # no factor at all (frame 0 without a prior, its IMU factor left out, nothing anchored in it -- fuzz seed 6139): m = 0 and n = 0 in the reference, too
    nimu = len(mw["imu"]["frame_i"])
    mw0 = dict(mw, imu={k: (np.asarray(v)[none] if isinstance(v, np.ndarray) and v.shape[:1] == (nimu,) else v) for k, v in mw["imu"].items()})
    W0m = gpu.Window(mw0)
    dr0 = [W0m.block_ptr("pose", 0), W0m.block_ptr("sb", 0)]
    h0 = C.c_void_p()
    gpu.check(L.tcv_marginalize(W0m.h, (gpu._dp * 2)(*dr0), 2, C.byref(h0)))
    P0 = gpu.Prior(h0)
    assert P0.dims() == (0, 0, 0, 0)
    As0, bs0 = P0.schur()
    assert As0.shape == (0, 0)
    # a prior built by hand with n = 0 (checkpoint of such a state)
    h2 = C.c_void_p()
    gpu.check(L.tcv_prior_create(C.byref(h2), 30, 0, 0, None, None, None, None, None))
    assert gpu.Prior(h2).dims() == (30, 0, 0, 0)
