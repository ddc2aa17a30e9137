"""GPU parity of the solve kernel's paths outside the big phases -- the per-solve J0'J0 of the prior in 2 x 2 blocks, the dogleg step
formed inside the Plus, the landmark slot loops that run four slots per trip -- on windows shaped to reach their edges: no landmark,
one landmark, landmarks with 2, 3 and 11 slots (remainder groups, and full groups plus a remainder), no prior, priors with an odd and
an even number of stored rows, with and without leading zero rows, a prior of one column, a 3-frame window.
Every case is one window through gpu_solve / check_against_oracle of tests/test_gpu_solve.py with their gates; check_against_oracle
compares first_step(k), which is made from the dogleg step the Plus applies.

(An IMU sqrt_info supplied by the caller is not among the cases: no entry point of the library hands one to the packer -- every call of
pack_problem passes none -- so the kernel always computes it.)"""
import numpy as np
import pytest

import synth
from test_gpu_solve import check_against_oracle, gpu_solve
from util import golden_windows, sub_window

pytestmark = pytest.mark.gpu


def keep_factors(w, keep):
    """the window with the point factors `keep` (indices) only; landmarks left without a factor are dropped"""
    pr = w["proj"]; n = len(pr["frame_i"])
    out = dict(w)
    out["proj"] = {k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in pr.items()}
    used = sorted(set(int(l) for l in out["proj"]["landmark"]))
    remap = {l: i for i, l in enumerate(used)}
    out["proj"]["landmark"] = np.array([remap[int(l)] for l in out["proj"]["landmark"]], int)
    out["lam"] = np.asarray(w["lam"])[used]
    return out


def leading_zero_rows(J0):
    k = 0
    while k < J0.shape[0] and not J0[k].any():
        k += 1
    return k


def solve_and_check(gpu, w, ex_constant=False):
    W, b, s = gpu_solve(gpu, [w], estimate_extrinsic=not ex_constant)
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 8, True, ex_constant=ex_constant)
    return W[0], b


def test_no_landmarks(gpu):
    w = dict(synth.window_at(synth.make_windows(910, 1), 0))
    w = keep_factors(w, [])
    assert len(w["lam"]) == 0
    solve_and_check(gpu, w)


def test_one_landmark(gpu):
    w = synth.window_at(synth.make_windows(911, 1), 0)
    lm = np.asarray(w["proj"]["landmark"])
    w = keep_factors(w, [k for k in range(len(lm)) if lm[k] == 0])
    assert len(w["lam"]) == 1
    solve_and_check(gpu, w)


def test_landmarks_with_2_3_and_11_slots(gpu):
    """With the extrinsic constant a landmark's slots are the poses it is seen from: its anchor frame and one per factor.  Landmark 0 is
    tracked through all eleven frames (11 slots); two others are cut to one and two factors (2 and 3 slots); the rest keep theirs (3 to 5)."""
    w = synth.window_at(synth.make_windows(912, 1), 0)
    lm = np.asarray(w["proj"]["landmark"])
    assert int((lm == 0).sum()) == 10
    seen = {}
    keep = []
    for k, l in enumerate(lm):
        seen[int(l)] = seen.get(int(l), 0) + 1
        if (int(l) == 1 and seen[1] > 1) or (int(l) == 2 and seen[2] > 2):
            continue
        keep.append(k)
    w = keep_factors(w, keep)
    lm = np.asarray(w["proj"]["landmark"])
    slots = [1 + len(set(int(f) for f in np.asarray(w["proj"]["frame_j"])[lm == l])) for l in range(3)]
    assert slots == [11, 2, 3]
    solve_and_check(gpu, w, ex_constant=True)


def test_no_prior(gpu):
    w = dict(synth.window_at(synth.make_windows(913, 1), 0), prior=None)
    solve_and_check(gpu, w)


def test_prior_with_an_odd_number_of_stored_rows(gpu):
    """the golden main window: n = 75 columns (the last 2 x 2 block of J0'J0 has one column), 34 leading zero rows, 41 stored"""
    pre, main, z = golden_windows()
    p = main["prior"]
    assert p["n"] == 75 and p["n"] - leading_zero_rows(np.asarray(p["J0"])) == 41
    solve_and_check(gpu, main)


def test_prior_without_zero_rows(gpu):
    """k0 = 0: the golden prior with its zero rows replaced by a weak diagonal (75 stored rows).  A one-window batch has the whole LDS of
    its CU, so J0 is staged in ONE piece here; the two-piece staging of such a prior (batches larger than the chip) and the paths that read
    J0 from global memory are the cases of tests/test_gpu_prior_paths.py."""
    pre, main, z = golden_windows()
    p = main["prior"]
    J0 = np.array(p["J0"], dtype=float)
    for i in range(leading_zero_rows(J0)):
        J0[i, i] = 1e-2
    assert leading_zero_rows(J0) == 0
    solve_and_check(gpu, dict(main, prior=dict(p, J0=J0)))


def test_first_generation_prior_from_the_batch(gpu):
    """the prior a batch's marginalisation leaves (b0.prior(k)), attached to the next window and linearised at its states"""
    w0 = synth.window_at(synth.make_windows(914, 1), 0)
    W0 = gpu.Window(w0)
    mw = gpu.margin_old_window(w0)
    M0 = gpu.Window(mw, share=W0)
    b0 = gpu.Batch([W0], [M0], [gpu.margin_old_drops(W0, mw)])
    b0.solve(gpu.default_options(8, True)); b0.marginalize(); b0.synchronize()
    Pr = b0.prior(0)
    d = Pr.export()
    d["blocks"] = gpu.shifted_prior_blocks(Pr, W0)
    nxt = synth.window_at(synth.make_windows(915, 1), 0)
    cur = {"pose": nxt["pose"], "sb": nxt["speedbias"]}
    d["x0"] = [np.array(cur[nm][i], dtype=float).copy() if nm in cur else np.array(nxt["ex_pose"], dtype=float).copy() for nm, i in d["blocks"]]
    assert d["n"] == 75 and len(d["blocks"]) == 12      # poses 0..9, speed-bias 0, extrinsic
    solve_and_check(gpu, dict(nxt, prior=d))


def test_prior_with_one_column(gpu):
    """n = 1: a prior on para_Td alone (one 2 x 2 block of J0'J0 with three of its entries outside the matrix)"""
    w = synth.with_time_offset(synth.window_at(synth.make_windows(916, 1), 0), 916)
    p = dict(m=0, n=1, sizes=[1], idx=[0], x0=[np.array([0.0])], J0=np.array([[40.0]]), r0=np.array([0.02]), blocks=[("td", 0)])
    w = dict(w, prior=p)
    import np_oracle as NO
    from util import fro, rel
    W = gpu.Window(w); b = gpu.Batch([W]); b.solve(gpu.default_options(8, True, True, 256, True)); b.synchronize(); b.download_states()
    s = b.summaries()[0]
    x, so = NO.solve(NO.Problem(w), 8, True)
    assert s.num_iterations == len(so["iterations"])
    assert abs(s.final_cost - so["final_cost"]) < 1e-6 * so["final_cost"]
    assert rel(W.pose, x["pose"]) < 1e-6 and rel(W.sb, x["sb"]) < 1e-6 and abs(W.td[0] - x["td"][0]) < 1e-6 * max(1e-3, abs(x["td"][0]))
    fo = np.asarray(so["iterations"][1]["delta"]); fg = b.first_step(0)
    assert len(fg) == len(fo) and fro(fg, fo) < 1e-6
    w_free = dict(w, prior=None)
    Wf = gpu.Window(w_free); bf = gpu.Batch([Wf]); bf.solve(gpu.default_options(8, True)); bf.synchronize(); bf.download_states()
    assert abs(Wf.td[0] - W.td[0]) > 1e-6      # the prior is really in the system


def test_three_frame_window(gpu):
    w = sub_window(synth.window_at(synth.make_windows(917, 1), 0), 3)
    solve_and_check(gpu, w)
