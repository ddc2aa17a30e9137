"""The residency paths of the marginalisation prior in the solve kernel, on the host: which path every case of tests/prior_path_cases.py
takes (pinned: part A in_lds / staged / global with the split nb | ns, setup lds / global with its column stride), that the oracle itself
tells the pieces of such a prior apart by far more than the gates of tests/test_gpu_prior_paths.py, and which paths a plan can take at all.

Reachability (test_chain_layout_never_takes_a_global_path; profiles/prior_paths.txt has the counts): over windows of 3 .. 11 frames with
0, 3, 50, 140, 200 and 279 landmarks, full-rank priors of up to 80 columns over the first p poses, one or two leading speed-bias blocks
and the extrinsic, in the plans of a plain batch and of the cooperative mode with four helpers (TCV_PLAN_COOP = 0, 4), NO plan in the
chain layout takes the `global` branch of part A or of the setup: a window whose pool is too small for the chain's working set is
laid out dense before that (the packer refused none of the 1464 plans).  Both `global` branches run in the dense layout only (short windows: the dense cases)."""
import os

import numpy as np
import pytest

import prior_path_cases as PC
import synth
from util import fro, sub_window

GATE_INITIAL_COST, GATE_FIRST_STEP, FACTOR = 1e-8, 1e-6, 1000.0      # the GPU test's gates on the two quantities; the sensitivity asked for


@pytest.fixture(scope="module")
def tcv(built):
    import tcv
    return tcv


@pytest.fixture(params=[0, 1], ids=["variant0", "variant1"])
def variant(request, tcv):
    tcv.check(tcv.lib().tcv_set_solver_variant(request.param))
    yield request.param
    tcv.check(tcv.lib().tcv_set_solver_variant(0))


def test_header_mirror_matches_the_packer(tcv):
    """plan_header's own guards, on a chain plan and a dense one; the kept zero rows follow tcv_packed.h (r0 counts too)"""
    w, exc = PC.chain_cases()["nr41_control"]
    h = PC.plan_header(tcv, tcv.Window(w))
    assert h.chain == 1 and h.prior_n == 75 and h.nland == 50 and h.n_frames == 11 and h.c_pool > h.c_stage_cap > 0
    wd, exc = PC.dense_cases()["f3_nr51"]
    hd = PC.plan_header(tcv, tcv.Window(wd))
    assert hd.chain == 0 and hd.prior_n == 51 and (hd.nt, hd.ntp) == (4, 2)
    J0 = np.zeros((4, 4)); J0[2, 1] = 1.0; r0 = np.zeros(4)
    assert PC.prior_zero_rows(J0, r0) == 2
    r0[1] = 1e-300
    assert PC.prior_zero_rows(J0, r0) == 1
    assert PC.prior_zero_rows(np.zeros((4, 4)), np.zeros(4)) == 3      # one row is kept


@pytest.mark.parametrize("name", list(PC.CHAIN_EXPECTED))
def test_chain_case_takes_its_path(tcv, name):
    w, exc = PC.chain_cases()[name]
    d = PC.case_paths(tcv, w, exc)
    print(name, d)
    assert d["layout"] == "chain"
    assert (d["part_a"], d["nb"], d["ns"], d["setup"]) == PC.CHAIN_EXPECTED[name], d
    if name == "nr75_L90_aligned":      # the split before the alignment fix would be 64 | 11: both nr and ns odd
        assert d["pcap"] + 1 == 64 and d["nr"] & 1
    if name == "nr55_one_piece":        # one piece of 4125 doubles; with dx and r behind it, 6 doubles more than the staging part of the pool
        assert d["nr"] * d["n"] == 4125 and 4126 + 2 * d["n"] == d["stage_cap"] + 6
    if name == "nr75_ex_constant":      # the constant columns (pcol < 0) lie in both pieces
        assert tcv.Window(w, estimate_extrinsic=False).plan_stats()["nc"] == 165
        lo = w["prior"]["idx"][w["prior"]["blocks"].index(("ex", 0))]
        assert lo < d["ns"] < lo + 6, (lo, d["ns"])


@pytest.mark.parametrize("name", list(PC.DENSE_EXPECTED))
def test_dense_case_takes_its_path(tcv, variant, name):
    w, exc = PC.dense_cases()[name]
    d = PC.case_paths(tcv, w, exc)
    print(variant, name, d)
    assert d["layout"] == "dense"      # no speed-bias chain is left: variant 0 packs it dense too
    assert (d["part_a"], d["setup"], d["ldj"]) == PC.DENSE_EXPECTED[name], d
    assert (d["nb"], d["ns"]) == (d["n"], 0)


@pytest.mark.parametrize("name", list(PC.CHAIN_EXPECTED) + list(PC.DENSE_EXPECTED))
def test_oracle_tells_the_pieces_of_the_prior_apart(name):
    """Oracle only.  Zeroing the columns of either piece of J0, or its last stored row, moves the oracle's initial cost or its first step
    by at least 1000 x the gate the GPU test puts on that quantity: a kernel that mishandles one piece cannot pass."""
    w, exc = (PC.chain_cases()[name] if name in PC.CHAIN_EXPECTED else PC.dense_cases()[name])
    ns = PC.CHAIN_EXPECTED[name][2] if name in PC.CHAIN_EXPECTED else 0
    c0, f0 = PC.oracle_first(w, exc)
    changes = PC.prior_changes(w, ns)
    assert len(changes) == (3 if ns else 2)
    for what, wc in changes.items():
        c1, f1 = PC.oracle_first(wc, exc)
        dc, df = abs(c1 - c0) / c0, fro(f1, f0)
        print("%-18s %-16s initial cost moves %.2e, first step %.2e" % (name, what, dc, df))
        assert dc >= FACTOR * GATE_INITIAL_COST or df >= FACTOR * GATE_FIRST_STEP, (name, what, dc, df)


# ---- reachability ----------------------------------------------------------------------------------------------------------------
SWEEP_LANDMARKS = (0, 3, 50, 140, 200, 279)


def _first_landmarks(w, n_land):
    """the window with its first n_land landmarks (and their factors) only"""
    pr = {k: np.asarray(v) if isinstance(v, (list, np.ndarray)) else v for k, v in w["proj"].items()}
    n = len(pr["landmark"])
    keep = pr["landmark"] < n_land
    out = dict(w, lam=np.asarray(w["lam"])[:n_land])
    out["proj"] = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in pr.items()}
    return out


def sweep(tcv):
    """(rows, counts): one row (coop, frames, landmarks, n, layout, part_a, setup) per accepted plan"""
    big = synth.window_at(synth.make_windows(5500, 1, n_landmarks=1024), 0)
    rows, refused = [], 0
    old = os.environ.get("TCV_PLAN_COOP")
    try:
        for coop in (0, 4):
            os.environ["TCV_PLAN_COOP"] = str(coop)
            for frames in range(3, 12):
                cut = sub_window(big, frames) if frames < 11 else dict(big, prior=None)
                for L in SWEEP_LANDMARKS:
                    w = _first_landmarks(cut, L)
                    assert len(w["lam"]) == L, (frames, L, len(w["lam"]))
                    for n_sb in (1, 2):
                        for poses in range(1, frames + 1):
                            n = 6 * poses + 9 * n_sb + 6
                            if n > 80:
                                continue
                            blocks = [("pose", i) for i in range(poses)] + [("sb", i) for i in range(n_sb)] + [("ex", 0)]
                            wp = dict(w, prior=PC.hand_prior(w, blocks, n, seed=n))
                            try:
                                d = PC.case_paths(tcv, wp)
                            except tcv.TcvError:
                                refused += 1
                                continue
                            rows.append((coop, frames, L, n, d["layout"], d["part_a"], d["setup"]))
    finally:
        if old is None:
            os.environ.pop("TCV_PLAN_COOP", None)
        else:
            os.environ["TCV_PLAN_COOP"] = old
    return rows, refused


def summarize(rows, refused):
    out = ["plans: %d accepted, %d refused by the packer" % (len(rows), refused)]
    for layout in ("chain", "dense"):
        for coop in (0, 4):
            sel = [r for r in rows if r[4] == layout and r[0] == coop]
            cnt = {}
            for r in sel:
                cnt[(r[5], r[6])] = cnt.get((r[5], r[6]), 0) + 1
            out.append("%s layout, TCV_PLAN_COOP=%d: %d plans; (part A, setup): %s" % (layout, coop, len(sel), ", ".join("%s/%s %d" % (a, s, c) for (a, s), c in sorted(cnt.items()))))
    return out


def test_chain_layout_never_takes_a_global_path(tcv):
    rows, refused = sweep(tcv)
    for line in summarize(rows, refused):
        print(line)
    chain = [r for r in rows if r[4] == "chain"]
    assert len(chain) > 300 and {r[0] for r in chain} == {0, 4} and {r[1] for r in chain} == set(range(3, 12))
    assert {r[2] for r in chain} >= {0, 3, 50, 140, 200} and max(r[3] for r in chain) >= 75
    assert {r[5] for r in chain} == {"in_lds", "staged"}, "a chain-layout plan takes part A's global path: give it a GPU case"
    assert {r[6] for r in chain} == {"lds"}, "a chain-layout plan takes the setup's global path: give it a GPU case"
