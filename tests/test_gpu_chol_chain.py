"""The dense tail of the solve kernel (csrc/tcv_solve.hip: diag_tile_wave_full, back_subst) after its pivot chain was shortened: a full
16-pivot tile runs branch-free, the pivot column reaches the trailing FMAs by DPP row broadcast (the identity rows take the matrix rows'
column through v_permlane16_swap), invdiag is stored once per tile, and the 16-step triangular solves of the back substitution broadcast
the same way.  The arithmetic is the parent's (profiles/chol_pivot_chain.txt: bit-identical outputs); here the shapes at the edges of the
new code run against the oracles.  The camera system of the chain layout is 6 F + 6 wide for F frames:

  f2     2 frames, 18 wide   one full tile, then a partial tile of 2 pivots: the full-tile body hands over to the loop with the k < cmax test
  f5     5 frames, 36 wide   two full tiles + 4
  f7     7 frames, 48 wide   exactly three full tiles; the fourth tile row holds the right-hand side only (no partial tile, the invdiag store
                             of the last full tile, back_subst starting on an empty pivot set)
  bench  four benchmark windows (11 frames, GPU-made n = 75 prior), 72 wide: four full tiles + 8
  relo   a relocalisation window, 78 wide: the kernel instance with ProjectionTdFactor (NumPy oracle: the C oracle has no such window)

Gates, all fixed figures of existing tests:
  tests/test_gpu_solve.py check_against_oracle: same iteration count, termination, dogleg cases and accepted steps as the C oracle; costs,
      final cost, states (whole and per family) and the first step to 1e-6, the model cost changes to 1e-5             (f5, f7, bench)
  tests/test_gpu_solve.py test_rank_deficient_windows_keep_the_oracles_accuracy, whose class a two-frame window without a prior is
      (held by the trust region's mu D^2 alone, condition ~1e9): first step to 1e-6, same accepted steps, final cost to 2e-5      (f2)
  tests/test_gpu_relo.py: iteration count, accepted steps, dogleg cases, final cost and every state block to 1e-6 against NumPy    (relo)
  tests/test_gpu_td.py test_td_window_in_cooperative_mode_gives_the_same_bits: the cooperative instance (1 + H workgroups) and the chain
      instance on the same plan (workgroups_per_window = 1) give the same bits -- the two translation units compile the factorisation
      separately
  bit for bit: a window in a batch larger than the chip (two workgroups per CU, 80 KiB of LDS each) against the same window in the small
      batch; its copies in the large batch, a second run and the reversed window order                            (f2, f5, f7, bench)
  tests/test_gpu_relo.py test_relocalisation_window_in_a_large_batch, the existing comparison of a relocalisation window alone (whole LDS,
      one visual chunk) with the same window in a batch of 300 (80 KiB: other chunks, another order of the sums in the LINEARISATION, so
      not the same bits): final cost, poses and the relocalisation pose to 1e-9; copies, second run and reversed order bit for bit   (relo)
The first step against the oracle is back_subst's result in the factored system; no separate residual check.
Every figure is printed before the case asserts.

The non-positive-pivot path (chol_tiles returns false, mu x 10, linearise again) is owned by tests/termination_cases.py and
tests/test_gpu_termination.py.  No window of the repository reaches it: in the C oracle's traces of the fuzzer's structures (seeds 0 .. 299
of tests/dev/fuzz_solve.py, the rank-deficient two-frame windows among them, 8 fixed iterations) and of every case of
tests/termination_cases.py no record's mu is above what the record before it gives (accepted: max(1e-8, mu / 5), rejected: mu, invalid
step: 10 mu), so there is no such case here either."""
import numpy as np
import pytest

import np_oracle as NO
import orc
import synth
from relo_util import add_relocalisation, hip_relo_window
from test_gpu_solve import TOL, check_against_oracle
from util import fro, rel, sub_window

pytestmark = pytest.mark.gpu

PACKED = 300          # more windows than CUs: the plain chain kernel, two workgroups per CU
RAGGED = {"f2": (2, 18), "f5": (5, 36), "f7": (7, 48)}
_CACHE = {}


def windows(gpu, name):
    """the case's windows (dicts), built once"""
    if name not in _CACHE:
        if name in RAGGED:
            _CACHE[name] = [sub_window(synth.window_at(synth.make_windows(400, 1), 0), RAGGED[name][0])]
        elif name == "bench":
            import bench
            _CACHE[name] = bench.build_batches(gpu, synth, 100000, 4)[1]
        else:
            _CACHE[name] = [add_relocalisation(dict(synth.window_at(synth.make_windows(9300, 1, with_lines=False), 0), prior=None), f=6, seed=2)]
    return _CACHE[name]


def make(gpu, w):
    """(tcv.Window, relocalisation pose or None)"""
    if "relo" in w:
        return hip_relo_window(gpu, w)
    return gpu.Window(w), None


def solve(gpu, wins, wg=0):
    made = [make(gpu, w) for w in wins]
    W = [m[0] for m in made]
    b = gpu.Batch(W)
    b.solve(gpu.default_options(8, True, True, 256, True, wg)); b.synchronize(); b.download_states()
    return W, [m[1] for m in made], b, b.summaries()


def bits(W, relo, s):
    n = s.num_iterations
    out = [W.pose.copy(), W.sb.copy(), W.ex.copy(), W.lam.copy(), np.array([s.cost[i] for i in range(n)]), np.array([s.final_cost])]
    if relo is not None:
        out.append(relo.copy())
    return out


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["f2", "f5", "f7", "bench", "relo"])
def test_shape_against_the_oracle(gpu, name):
    wins = windows(gpu, name)
    W, relo, b, s = solve(gpu, wins)
    ps = b.plan_stats()
    st = W[0].plan_stats()
    print("%s: layout %s, nc %s, pose system %s wide, cooperative %s" % (name, ps["layout"], st.get("nc"), st.get("npp"), b.cooperative()))
    assert ps["layout"] == "chain", (name, "dense layout", st)
    if name in RAGGED:
        assert st["npp"] == RAGGED[name][1], st
    elif name == "bench":
        assert st["npp"] == 72, st
    else:
        assert st["npp"] == 78 and st["nc"] == 177, st
    for k, w in enumerate(wins):
        if name == "relo":
            x, so = NO.solve(NO.Problem(w), 8, True)
            its = so["iterations"]
            fo = np.asarray(its[1]["delta"]); fg = b.first_step(k)
            err = {key: rel(got, x[key]) for key, got in (("pose", W[k].pose), ("sb", W[k].sb), ("ex", W[k].ex), ("lam", W[k].lam), ("relo", relo[k]))}
            print("relo: iterations %d / %d, final cost %.3e rel, first step %.3e (%d / %d long), states %s"
                  % (s[k].num_iterations, len(its), abs(s[k].final_cost - so["final_cost"]) / so["final_cost"], fro(fg[:len(fo)], fo[:len(fg)]), len(fg), len(fo),
                     {key: float("%.2e" % v) for key, v in err.items()}))
            assert s[k].num_iterations == len(its)
            assert [bool(s[k].step_ok[i]) for i in range(1, len(its))] == [bool(r.get("step_ok", False)) for r in its[1:]]
            assert [s[k].dogleg_case[i] for i in range(1, len(its))] == [int(r.get("dogleg_case", r.get("case", -1))) for r in its[1:]]
            assert abs(s[k].final_cost - so["final_cost"]) < 1e-6 * so["final_cost"]
            assert all(v < 1e-6 for v in err.values()), err
            assert len(fg) == len(fo) and fro(fg, fo) < TOL
        elif name == "f2":
            O = orc.Window(w); so = O.solve(8, True)
            fo = np.array(so.first_delta[:so.n_local]); fg = b.first_step(k)
            n = so.num_iterations
            print("f2: first step %.3e, iterations %d / %d, final cost %.6e / %.6e (rel %.3e), states (not gated) %s"
                  % (fro(fg, fo), s[k].num_iterations, n, s[k].final_cost, so.final_cost, abs(s[k].final_cost - so.final_cost) / max(so.final_cost, 1e-12),
                     {key: float("%.2e" % rel(W[k].states()[key], O.states()[key])) for key in ("pose", "sb", "ex", "lam")}))
            assert len(fg) == len(fo) and fro(fg, fo) < TOL
            assert s[k].num_iterations == n and [s[k].step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
            assert abs(s[k].final_cost - so.final_cost) < 2e-5 * max(so.final_cost, 1e-12)
        else:
            O = orc.Window(w); so = O.solve(8, True)
            print("%s[%d]: first step %.3e, final cost rel %.3e, states %s" % (name, k, fro(b.first_step(k), np.array(so.first_delta[:so.n_local])),
                  abs(s[k].final_cost - so.final_cost) / so.final_cost, {key: float("%.2e" % rel(W[k].states()[key], O.states()[key])) for key in ("pose", "sb", "ex", "lam")}))
            check_against_oracle(gpu, w, W[k], b, s[k], k, 8, True)


@pytest.mark.parametrize("name", ["f2", "f5", "f7", "bench", "relo"])
def test_same_bits_in_every_launch_shape(gpu, name):
    wins = windows(gpu, name)
    n = len(wins)
    # a handful of windows: the cooperative instance, and the chain instance on the same plan
    alone = {}
    for wg in ((1,) if name == "relo" else (0, 1)):      # (the cooperative mode does not take relocalisation windows)
        W, relo, b, s = solve(gpu, wins, wg)
        co = b.cooperative()
        alone[wg] = [bits(W[k], relo[k], s[k]) for k in range(n)]
        print("%s, %d window(s), workgroups_per_window %d: %s" % (name, n, wg, co))
        if wg == 1:
            assert co["last_solve_workgroups"] == 1, co
        else:
            # (a short window gets no helper workgroups: the benchmark windows must get some)
            assert co["last_solve_workgroups"] == 1 + co["helpers"] and (co["helpers"] >= 1 or name != "bench"), co
    if 0 in alone:
        assert all(same_bits(alone[0][k], alone[1][k]) for k in range(n)), "cooperative instance against the chain instance on the same plan"
    # a batch larger than the chip: copies of the same windows, twice, and in reversed order
    order = [k % n for k in range(PACKED)]
    runs = []
    for rev in (False, False, True):
        o = order[::-1] if rev else order
        W, relo, b, s = solve(gpu, [wins[k] for k in o])
        assert b.cooperative()["last_solve_workgroups"] == 1 and b.plan_stats()["grid"] == PACKED, (b.cooperative(), b.plan_stats())
        got = [bits(W[i], relo[i], s[i]) for i in range(PACKED)]
        runs.append(got[::-1] if rev else got)
    for i in range(PACKED):
        assert same_bits(runs[0][i], runs[0][order[i]]), ("copies in one batch", i)
        assert same_bits(runs[0][i], runs[1][i]), ("second run", i)
        assert same_bits(runs[0][i], runs[2][i]), ("reversed order", i)
    worst = [0.0, 0.0]
    exact = True
    for k in range(n):
        a, p = alone[1][k], runs[0][k]
        worst[0] = max(worst[0], abs(a[5][0] - p[5][0]) / a[5][0])
        worst[1] = max([worst[1]] + [rel(p[i], a[i]) for i in (0, 1, 3)] + ([rel(p[6], a[6])] if name == "relo" else []))
        exact = exact and same_bits(a, p)
    print("%s: small batch against the batch of %d: same bits %s, final cost %.2e, states %.2e" % (name, PACKED, exact, worst[0], worst[1]))
    if name == "relo":
        assert worst[0] < 1e-9 and worst[1] < 1e-9, worst
    else:
        assert exact, worst
