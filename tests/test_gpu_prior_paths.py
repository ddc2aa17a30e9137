"""GPU parity of the solve kernel's prior phases on every residency path (tests/prior_path_cases.py names them; tests/test_prior_paths_cpu.py
pins the path of every case below and shows that the oracle tells the pieces of each prior apart by 1000 x these gates).

  chain batch      300 windows -- the cases among cheap fillers --, two workgroups per CU on 80 KiB each, no helpers: the plan
                   tcv_problem_plan_ints shows.  in_lds (nr = 41, 54) and staged: one piece (nr = 55), ns = 1, 2, 8, 10, the alignment
                   decrement (ns = 12 at 90 landmarks), constant columns inside both pieces (extrinsic held constant), the TD instance
                   of the chain kernel (a full-rank prior that holds para_Td, n = 76).
  dense batch      3- and 4-frame windows with a prior over every block, under both solver variants: part A global with the setup in LDS
                   (padded and unpadded column stride) and both global.
  one-piece batch  the chain cases again in a batch smaller than the chip, one workgroup per window, the whole LDS: J0 in one piece.

Every case passes check_against_oracle of tests/test_gpu_solve.py with its gates (iterations, accept / reject and dogleg sequence, costs,
states, first step, model cost change) and has its initial cost within 1e-8 of the oracle's (the gate of tests/test_gpu_marg.py); the
ESTIMATE_TD case is held to the same gates against np_oracle (the C oracle has no ProjectionTdFactor).  profiles/prior_paths.txt has the
measured figures.  The two policies are not compared bit for bit (the visual chunking differs too); with ns = 1 the staged path adds
the odd columns of J0 in the accumulator that holds the even ones on the one-piece path, so that case would differ in any event."""
import numpy as np
import pytest

import np_oracle as NO
import orc
import prior_path_cases as PC
from test_gpu_solve import TOL, check_against_oracle, check_states_by_family
from util import fro, rel, rel_by_family, state_families

pytestmark = pytest.mark.gpu
GATE_INITIAL_COST = 1e-8
CHAIN, DENSE = list(PC.CHAIN_EXPECTED), list(PC.DENSE_EXPECTED)
REPORT = []
_NP = {}


def np_solution(w):
    """np_oracle's solve of an ESTIMATE_TD case, computed once"""
    if id(w) not in _NP:
        _NP[id(w)] = (w, NO.solve(NO.Problem(w), 8, True))
    return _NP[id(w)][1]


def solve_batch(gpu, wins, ex_constant, workgroups_per_window=0, before=None):
    W = [gpu.Window(w, estimate_extrinsic=not exc) for w, exc in zip(wins, ex_constant)]
    b = gpu.Batch(W)
    if before is not None:
        before(b)
    b.solve(gpu.default_options(8, True, True, 256, True, workgroups_per_window)); b.synchronize(); b.download_states()
    return W, b, b.summaries()


def check_against_np_oracle(w, W, b, s, k):
    """check_against_oracle with np_oracle on the other side: the same quantities, the same gates, and para_Td among the states"""
    x, so = np_solution(w)
    its = so["iterations"]
    n = len(its)
    assert s.num_iterations == n and s.termination == so["termination_code"]
    assert [s.dogleg_case[i] for i in range(1, n)] == [int(r["case"]) for r in its[1:]]
    assert [s.step_ok[i] for i in range(1, n)] == [int(bool(r["step_ok"])) for r in its[1:]]
    assert rel([s.cost[i] for i in range(n)], [r["cost"] for r in its]) < TOL
    assert abs(s.final_cost - so["final_cost"]) < TOL * so["final_cost"]
    sg = W.states()
    for key in ("pose", "sb", "ex", "lam", "td"):
        assert rel(sg[key], x[key]) < TOL, key
    check_states_by_family(sg, x)
    fo = np.asarray(its[1]["delta"]); fg = b.first_step(k)
    assert len(fg) == len(fo) and fro(fg, fo) < TOL
    assert rel([s.model_cost_change[i] for i in range(1, n)], [r["model_cost_change"] for r in its[1:]]) < 1e-5


def figures(w, exc, W, b, s, k):
    """measured relative errors against the oracle: initial cost, first step, solved states (worst family)"""
    if w.get("td") is not None:
        x, so = np_solution(w)
        c0, f0 = so["initial_cost"], np.asarray(so["iterations"][1]["delta"])
    else:
        O = orc.Window(w, ex_constant=exc); so = O.solve(8, True)
        x, c0, f0 = O.states(), so.initial_cost, np.array(so.first_delta[:so.n_local])
    fg = b.first_step(k)
    byf = rel_by_family(state_families(W.states()), state_families(x))
    return dict(initial_cost=abs(s.initial_cost - c0) / c0, first_step=fro(fg, f0) if len(fg) == len(f0) else float("inf"), states=max(byf.values()))


def check_case(gpu, run, name, cases, tag, paths):
    w, exc = cases[name]
    W, b, s, k = run[name]
    f = figures(w, exc, W, b, s, k)
    line = "%-15s %-17s %-34s initial cost %.1e  first step %.1e  states %.1e" % (tag, name, paths, f["initial_cost"], f["first_step"], f["states"])
    print(line); REPORT.append(line)
    if w.get("td") is not None:
        check_against_np_oracle(w, W, b, s, k)
    else:
        check_against_oracle(gpu, w, W, b, s, k, 8, True, ex_constant=exc)
    assert f["initial_cost"] < GATE_INITIAL_COST, f


# ---- chain batch: two workgroups per CU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_per_cu(gpu):
    cases = PC.chain_cases()
    wins = PC.fillers(300 - len(CHAIN))
    at = {}
    for i, name in enumerate(CHAIN):      # the cases spread over the batch
        at[name] = 7 + 29 * i
        wins.insert(at[name], cases[name][0])
    exc = [False] * 300
    for name in CHAIN:
        assert wins[at[name]] is cases[name][0]
        exc[at[name]] = cases[name][1]

    def before(b):      # a changed policy must not route the cases to the one-piece path unnoticed
        st = b.plan_stats()
        assert st["layout"] == "chain" and st["lds_bytes"] == 81920, st
        assert b.cooperative()["helpers"] == 0, b.cooperative()
    W, b, s = solve_batch(gpu, wins, exc, before=before)
    return {name: (W[k], b, s[k], k) for name, k in at.items()}


@pytest.mark.parametrize("name", CHAIN)
def test_chain_batch_two_workgroups_per_cu(gpu, two_per_cu, name):
    e = PC.CHAIN_EXPECTED[name]
    check_case(gpu, two_per_cu, name, PC.chain_cases(), "two per CU", "%s nb %d ns %d, setup %s" % e)


# ---- the same cases, J0 in one piece ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_piece(gpu):
    cases = PC.chain_cases()

    def before(b):
        st = b.plan_stats()
        assert st["layout"] == "chain" and st["lds_bytes"] == 163840, st
    W, b, s = solve_batch(gpu, [cases[n][0] for n in CHAIN], [cases[n][1] for n in CHAIN], workgroups_per_window=1, before=before)
    assert b.cooperative()["last_solve_workgroups"] == 1, b.cooperative()      # cooperative mode off
    return {name: (W[k], b, s[k], k) for k, name in enumerate(CHAIN)}


@pytest.mark.parametrize("name", CHAIN)
def test_chain_cases_in_one_piece(gpu, one_piece, two_per_cu, name):
    check_case(gpu, one_piece, name, PC.chain_cases(), "one per CU", "in_lds (whole LDS)")
    a, c = state_families(one_piece[name][0].states()), state_families(two_per_cu[name][0].states())
    line = "%-15s %-17s largest state difference between the two policies %.1e" % ("", name, max(rel_by_family(a, c).values()))
    print(line); REPORT.append(line)


# ---- dense layout: the global paths ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1], ids=["variant0", "variant1"])
def dense_run(request, gpu):
    cases = PC.dense_cases()

    def before(b):      # the dense kernel's choice follows from the window's structure alone (tile counts, n, k0): no LDS policy enters it
        assert b.plan_stats()["layout"] == "dense", b.plan_stats()
    gpu.check(gpu.lib().tcv_set_solver_variant(request.param))
    try:
        W, b, s = solve_batch(gpu, [cases[n][0] for n in DENSE], [cases[n][1] for n in DENSE], before=before)
    finally:
        gpu.check(gpu.lib().tcv_set_solver_variant(0))
    return request.param, {name: (W[k], b, s[k], k) for k, name in enumerate(DENSE)}


@pytest.mark.parametrize("name", DENSE)
def test_dense_batch(gpu, dense_run, name):
    variant, run = dense_run
    e = PC.DENSE_EXPECTED[name]
    check_case(gpu, run, name, PC.dense_cases(), "dense variant %d" % variant, "%s, setup %s ldj %s" % e)


def test_zz_report():
    for line in REPORT:
        print(line)
