"""The chain elimination of the solve kernel (csrc/tcv_solve.hip: chain_forward, chain_mfma_share) after the tile pairs of S -= W'W were
shared out: wave 3 takes trips (two pairs each) behind its T step where the pairs outweigh it, half of them in the interval without a
T step, and the drain -- the update with the last W alone -- goes over all four wavefronts.  The pairs of one update touch disjoint tiles,
so the arithmetic is the parent's (profiles/chain_step_balance.txt: bit-identical outputs); here every shape of the schedule runs
against the oracles and against itself in every launch shape.  Active 16-column tile rows of W / pairs of the largest update / trips:

  f2      2 frames, 18 wide       2 rows, 3 pairs, 2 trips: the first T step, the interval without a T step and the drain are all of the chain
  f5      5 frames, 36 wide       3 rows, 6 pairs, 3 trips: an even count of pairs
  f7      7 frames, 48 wide       4 rows, 10 pairs, 5 trips
  bench   four benchmark windows (11 frames, device-made n = 75 prior), 72 wide: 5 rows, 15 pairs (odd: the left-over pair), 8 trips -- wave 3
          takes two behind its T step -- with the prior-coupled block last
  nop     the same 11 frames without a prior
  broken  a window whose IMU chain is broken (the constructor of tests/test_gpu_solve.py test_chain_layout_variants_vs_oracle): the second
          chain starts with fewer active tile rows than the first ended with
  td      an ESTIMATE_TD window: the kernel instance with ProjectionTdFactor (NumPy oracle)
  relo    a relocalisation window, 78 wide, on the same instance (NumPy oracle: the C oracle has no such window)

Gates, all fixed figures of existing tests:
  tests/test_gpu_solve.py check_against_oracle (TOL = 1e-6; model cost changes 1e-5)                                   (f5, f7, bench, nop)
  tests/test_gpu_solve.py test_rank_deficient_windows_keep_the_oracles_accuracy's class, as tests/test_gpu_chol_chain.py applies it:
      first step to 1e-6, same accepted steps, final cost to 2e-5                                                       (f2)
  tests/test_gpu_solve.py test_chain_layout_variants_vs_oracle: final cost, poses, speed-bias blocks and every state family to 1e-6,
      same dogleg cases                                                                                                  (broken)
  tests/test_gpu_td.py test_td_window_solve_vs_oracle: iterations, accepted steps, final cost, poses, speed-bias blocks and td to 1e-6,
      inverse depths to 1e-5, initial cost to 1e-9                                                                       (td)
  tests/test_gpu_relo.py / tests/test_gpu_chol_chain.py: iterations, accepted steps, dogleg cases, final cost, every state block to 1e-6  (relo)
  bit for bit: the cooperative instance (1 + H workgroups) against the chain instance on the same plan (workgroups_per_window = 1); the
      small batch against the same windows in a batch of 300 (two workgroups per CU); copies within the large batch, a second run, the
      reversed window order.  The two windows of the ProjectionTdFactor instance compare small against large to 1e-9 as
      tests/test_gpu_relo.py test_relocalisation_window_in_a_large_batch does (whole LDS against 80 KiB: another order of the sums in
      the linearisation), everything else bit for bit; the cooperative mode does not take relocalisation windows.
Every figure is printed before the case asserts."""
import numpy as np
import pytest

import np_oracle as NO
import orc
import synth
from relo_util import add_relocalisation, hip_relo_window
from test_gpu_solve import TOL, check_against_oracle, check_states_by_family
from util import fro, golden_windows, rel, sub_window

pytestmark = pytest.mark.gpu

PACKED = 300          # more windows than CUs: the plain chain kernel, two workgroups per CU
NPP = {"f2": 18, "f5": 36, "f7": 48, "bench": 72, "nop": 72, "broken": 72, "td": 73, "relo": 78}
NAMES = list(NPP)
TD_INSTANCE = ("td", "relo")
_CACHE = {}


def windows(gpu, name):
    """the case's windows (dicts), built once"""
    if name not in _CACHE:
        if name in ("f2", "f5", "f7"):
            _CACHE[name] = [sub_window(synth.window_at(synth.make_windows(400, 1), 0), int(name[1:]))]
        elif name == "bench":
            import bench
            _CACHE[name] = bench.build_batches(gpu, synth, 100000, 4)[1]
        elif name == "nop":
            _CACHE[name] = [dict(synth.window_at(synth.make_windows(400, 1), 0), prior=None)]
        elif name == "broken":
            pre = golden_windows()[0]
            im = dict(pre["imu"]); sd = np.array(im["sum_dt"], dtype=float).copy(); sd[4] = 11.0; im["sum_dt"] = sd
            _CACHE[name] = [dict(pre, imu=im)]
        elif name == "td":
            _CACHE[name] = [synth.with_time_offset(synth.window_at(synth.make_windows(41, 1), 0), 41, TR=0.02)]
        else:
            _CACHE[name] = [add_relocalisation(dict(synth.window_at(synth.make_windows(9300, 1, with_lines=False), 0), prior=None), f=6, seed=2)]
    return _CACHE[name]


def solve(gpu, wins, wg=0):
    made = [hip_relo_window(gpu, w) if "relo" in w else (gpu.Window(w), None) for w in wins]
    W = [m[0] for m in made]
    b = gpu.Batch(W)
    b.solve(gpu.default_options(8, True, True, 256, True, wg)); b.synchronize(); b.download_states()
    return W, [m[1] for m in made], b, b.summaries()


def bits(W, relo, s, td):
    n = s.num_iterations
    out = [W.pose.copy(), W.sb.copy(), W.ex.copy(), W.lam.copy(), np.array([s.cost[i] for i in range(n)]), np.array([s.final_cost])]
    if relo is not None:
        out.append(relo.copy())
    if td:
        out.append(np.array(W.td, dtype=float).copy())
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_shape_against_the_oracle(gpu, name):
    wins = windows(gpu, name)
    W, relo, b, s = solve(gpu, wins)
    ps = b.plan_stats()
    st = W[0].plan_stats()
    print("%s: layout %s, nc %s, pose system %s wide, cooperative %s" % (name, ps["layout"], st.get("nc"), st.get("npp"), b.cooperative()))
    assert ps["layout"] == "chain", (name, "dense layout", st)
    assert st["npp"] == NPP[name], st
    for k, w in enumerate(wins):
        if name in TD_INSTANCE:
            x, so = NO.solve(NO.Problem(w), 8, True)
            its = so["iterations"]
            got = [("pose", W[k].pose), ("sb", W[k].sb), ("lam", W[k].lam)] + ([("ex", W[k].ex), ("relo", relo[k])] if name == "relo" else [])
            err = {key: rel(g, x[key]) for key, g in got}
            print("%s: iterations %d / %d, initial cost %.3e rel, final cost %.3e rel, states %s"
                  % (name, s[k].num_iterations, len(its), abs(s[k].initial_cost - so["initial_cost"]) / so["initial_cost"],
                     abs(s[k].final_cost - so["final_cost"]) / so["final_cost"], {key: float("%.2e" % v) for key, v in err.items()}))
            assert s[k].num_iterations == len(its)
            assert [bool(s[k].step_ok[i]) for i in range(1, len(its))] == [bool(r.get("step_ok", False)) for r in its[1:]]
            assert abs(s[k].final_cost - so["final_cost"]) < 1e-6 * so["final_cost"]
            if name == "td":
                print("td: %.9e against %.9e" % (W[k].td[0], x["td"][0]))
                assert abs(s[k].initial_cost - so["initial_cost"]) < 1e-9 * so["initial_cost"]
                assert err["pose"] < 1e-6 and err["sb"] < 1e-6 and err["lam"] < 1e-5, err
                assert abs(W[k].td[0] - x["td"][0]) < 1e-6 * max(1e-3, abs(x["td"][0]))
            else:
                fo = np.asarray(its[1]["delta"]); fg = b.first_step(k)
                print("relo: first step %.3e (%d / %d long)" % (fro(fg[:len(fo)], fo[:len(fg)]), len(fg), len(fo)))
                assert [s[k].dogleg_case[i] for i in range(1, len(its))] == [int(r.get("dogleg_case", r.get("case", -1))) for r in its[1:]]
                assert all(v < 1e-6 for v in err.values()), err
                assert len(fg) == len(fo) and fro(fg, fo) < TOL
            continue
        O = orc.Window(w); so = O.solve(8, True); sto = O.states()
        fo = np.array(so.first_delta[:so.n_local]); fg = b.first_step(k)
        n = so.num_iterations
        print("%s[%d]: first step %.3e, iterations %d / %d, final cost %.6e / %.6e (rel %.3e), states %s"
              % (name, k, fro(fg, fo), s[k].num_iterations, n, s[k].final_cost, so.final_cost, abs(s[k].final_cost - so.final_cost) / max(so.final_cost, 1e-12),
                 {key: float("%.2e" % rel(W[k].states()[key], sto[key])) for key in ("pose", "sb", "ex", "lam")}))
        if name == "f2":
            assert len(fg) == len(fo) and fro(fg, fo) < TOL
            assert s[k].num_iterations == n and [s[k].step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
            assert abs(s[k].final_cost - so.final_cost) < 2e-5 * max(so.final_cost, 1e-12)
        elif name == "broken":
            assert abs(s[k].final_cost - so.final_cost) < 1e-6 * so.final_cost
            assert [s[k].dogleg_case[i] for i in range(9)] == [so.dogleg_case[i] for i in range(9)]
            assert rel(W[k].pose, sto["pose"]) < 1e-6 and rel(W[k].sb, sto["sb"]) < 1e-6
            check_states_by_family(W[k].states(), sto, 1e-6, name)
        else:
            check_against_oracle(gpu, w, W[k], b, s[k], k, 8, True)


@pytest.mark.parametrize("name", NAMES)
def test_same_bits_in_every_launch_shape(gpu, name):
    wins = windows(gpu, name)
    n = len(wins)
    td = name == "td"
    # a handful of windows: the cooperative instance, and the chain instance on the same plan
    alone = {}
    for wg in ((1,) if name == "relo" else (0, 1)):      # (the cooperative mode does not take relocalisation windows)
        W, relo, b, s = solve(gpu, wins, wg)
        co = b.cooperative()
        alone[wg] = [bits(W[k], relo[k], s[k], td) for k in range(n)]
        print("%s, %d window(s), workgroups_per_window %d: %s" % (name, n, wg, co))
        if wg == 1:
            assert co["last_solve_workgroups"] == 1, co
        else:
            assert co["last_solve_workgroups"] == 1 + co["helpers"] and (co["helpers"] >= 1 or name != "bench"), co
    if 0 in alone:
        eq = all(same_bits(alone[0][k], alone[1][k]) for k in range(n))
        print("%s: cooperative instance against the chain instance on the same plan: same bits %s" % (name, eq))
        assert eq
    # a batch larger than the chip: copies of the same windows, twice, and in reversed order
    order = [k % n for k in range(PACKED)]
    runs = []
    for rev in (False, False, True):
        o = order[::-1] if rev else order
        W, relo, b, s = solve(gpu, [wins[k] for k in o])
        assert b.cooperative()["last_solve_workgroups"] == 1 and b.plan_stats()["grid"] == PACKED, (b.cooperative(), b.plan_stats())
        got = [bits(W[i], relo[i], s[i], td) for i in range(PACKED)]
        runs.append(got[::-1] if rev else got)
    bad = [sum(not same_bits(runs[0][i], other(i)) for i in range(PACKED))
           for other in (lambda i: runs[0][order[i]], lambda i: runs[1][i], lambda i: runs[2][i])]
    worst = [0.0, 0.0]
    exact = True
    for k in range(n):
        a, p = alone[1][k], runs[0][k]
        worst[0] = max(worst[0], abs(a[5][0] - p[5][0]) / a[5][0])
        worst[1] = max([worst[1]] + [rel(p[i], a[i]) for i in (0, 1, 3)] + [rel(p[i], a[i]) for i in range(6, len(a))])
        exact = exact and same_bits(a, p)
    print("%s: windows of %d that differ from their copy / second run / reversed order: %s; small batch against the batch: same bits %s, final cost %.2e, states %.2e"
          % (name, PACKED, bad, exact, worst[0], worst[1]))
    assert bad == [0, 0, 0], bad
    if name in TD_INSTANCE:
        assert worst[0] < 1e-9 and worst[1] < 1e-9, worst
    else:
        assert exact, worst
