"""The termination cases of tests/termination_cases.py on the two oracles alone (no device): what makes them safe to gate the device on
(tests/test_gpu_termination.py).  For every case

  * np_oracle and the C oracle agree on termination, num_iterations, step_ok and dogleg_case;
  * a convergence decision is clear: the deciding quantity is <= 0.5 x its threshold at the deciding record, and at every earlier record
    dx_norm / (1e-8 (x_norm + 1e-8)), |cost change| / (1e-6 cost) and gradient_max_norm / 1e-10 are all >= 2 (a case that does not meet
    this is replaced, the bound stays);
  * the C oracle's own trace is unchanged under the three 1e-13 state perturbations of fuzz_solve.oracle_sensitivity;
  * check_trace_rules holds on both oracles' summaries (the checker is proven here before it judges the device).

Two exceptions, both stated by the arithmetic.  `radius` halves its radius 121 times at one state: from the record where the model's cost
change falls below 1e-12 x cost (4500 ulps of the cost, record 50 of 124) the numerator of rho is the rounding of two cost evaluations a few
ulps apart, so accept / reject is noise there -- np_oracle accepts a step at record 57 (rho 0.094) that the C oracle rejects (rho 0), and
the C oracle's own trace moves in 3 of 3 perturbations.  The two oracles are held to the same decisions above that line, and to termination
and num_iterations as a whole; the stability condition does not apply.  `long_trace_seed17` (200 landmarks, 100 iterations) takes
np_oracle a minute: it is compared with the C oracle over the first 10 iterations, which are the same arithmetic as the first 10 of the
100, and the C oracle runs all of them.

The margins are printed (run with -s)."""
import numpy as np
import pytest

import np_oracle as NO
import orc
import termination_cases as tc
from util import fmt_families, rel_by_family, state_families

NAMES = list(tc.EXPECTED)
CONVERGENCE = [n for n in NAMES if n not in tc.LONG_TRACE and n != "radius"]
NP_PREFIX = {"long_trace_seed17": 10}      # iterations np_oracle runs where the whole run is too slow for a test
_SOLVED = {}


def solved(name):
    """(C summary, C states, np summary or None, np states) of a case, each solve run once"""
    if name not in _SOLVED:
        w_hip, w_orc, exc, iters, fixed = tc.cases()[name]
        O = orc.Window(w_orc, ex_constant=exc); so = O.solve(iters, fixed)
        x, sn = NO.solve(NO.Problem(w_orc, ex_constant=exc), NP_PREFIX.get(name, iters), fixed)
        _SOLVED[name] = (so, O.states(), sn, x)
    return _SOLVED[name]


@pytest.mark.parametrize("name", NAMES)
def test_both_oracles_end_where_the_case_says(name):
    so, st, sn, x = solved(name)
    term, records = tc.EXPECTED[name]
    assert (so.num_iterations, so.termination) == (records, term)
    c, n = tc.trace_of(so), tc.np_trace_of(sn)
    if name in NP_PREFIX:
        k = NP_PREFIX[name]
        assert n[0] == k + 1 and n[1] == tc.NO_CONVERGENCE and n[2] == c[2][:k] and n[3] == c[3][:k]
    elif name == "radius":
        well_posed = [i for i in range(1, records) if so.model_cost_change[i] >= 1e-12 * so.cost[i]]
        k = well_posed[-1]
        assert well_posed == list(range(1, k + 1)) and k >= 40, k
        assert n[:2] == c[:2] and n[2][:k] == c[2][:k] and n[3][:k] == c[3][:k]
        print("%s: the oracles agree over the %d records whose model cost change is >= 1e-12 x cost" % (name, k))
    else:
        assert n == c
    if name not in NP_PREFIX:      # (printed, not gated: how far the two oracles' own solved states are apart)
        print("%-18s the two oracles' states apart: %s" % (name, fmt_families(rel_by_family(state_families(x), state_families(st)))))


@pytest.mark.parametrize("name", CONVERGENCE)
def test_convergence_decisions_are_clear(name):
    so, st, sn, x = solved(name)
    deciding, least = tc.check_margins(sn)
    print("%-18s ends on %d after %3d records: deciding quantity %.3g x its threshold, smallest earlier quantity %.3g x" %
          (name, sn["termination_code"], len(sn["iterations"]), deciding, least))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "radius"])
def test_the_oracles_trace_is_stable_under_state_noise(name):
    so, st, sn, x = solved(name)
    w_hip, w_orc, exc, iters, fixed = tc.cases()[name]
    for rep in range(3):
        s2 = orc.Window(tc.perturbed(w_orc, rep), ex_constant=exc).solve(iters, fixed)
        assert tc.trace_of(s2) == tc.trace_of(so), rep


@pytest.mark.parametrize("name", NAMES)
def test_trace_rules_hold_on_the_oracles_own_summaries(name):
    so, st, sn, x = solved(name)
    tc.check_trace_rules(so, so.num_iterations)
    tc.check_trace_rules(tc.np_summary(sn), len(sn["iterations"]))


def test_trace_rules_notice_a_wrong_summary():
    """the checker is not vacuous: one changed field of a correct summary fails it"""
    so, st, sn, x = solved("parameter_main")
    n = so.num_iterations
    tc.check_trace_rules(so, n)
    rej = next(i for i in range(1, n - 1) if not so.step_ok[i])
    acc = next(i for i in range(2, n - 1) if so.step_ok[i])
    c3 = next(i for i in range(1, n) if so.dogleg_case[i] == 3)

    def broken(field, i, value):
        s = tc.np_summary(sn)      # (a copy in plain lists)
        for f in ("cost", "cost_candidate", "model_cost_change", "radius", "mu", "rho", "step_norm", "step_ok", "dogleg_case"):
            setattr(s, f, [getattr(so, f)[k] for k in range(n)])
        s.initial_cost, s.final_cost = so.initial_cost, so.final_cost
        tc.check_trace_rules(s, n)
        getattr(s, field)[i] = value
        with pytest.raises(AssertionError):
            tc.check_trace_rules(s, n)
    broken("step_ok", rej, 1)
    broken("rho", acc, so.rho[acc] * (1 + 1e-9))
    broken("cost", rej, so.cost_candidate[rej])
    broken("radius", rej + 1, so.radius[rej])
    broken("radius", acc + 1, so.radius[acc + 1] * 2)
    broken("mu", acc, 1e-7)
    broken("step_norm", c3, so.step_norm[c3] * (1 + 1e-6))
    broken("model_cost_change", acc, -so.model_cost_change[acc])


def test_only_the_landmark_part_of_the_gradient_is_above_the_tolerance_at_entry():
    """gradient_landmarks_only: camera part <= 0.5 x the gradient tolerance, landmark part >= 2 x -- a gradient test without the landmark
    entries ends this case before its first iteration (1 record, termination 1) instead of after 2 records on the function tolerance"""
    w = tc.cases()["gradient_landmarks_only"][0]
    cam, lam = tc.gradient_parts(w)
    print("gradient_landmarks_only at entry: camera part %.3g x the gradient tolerance, landmark part %.3g x" % (cam / tc.GRADIENT_TOLERANCE, lam / tc.GRADIENT_TOLERANCE))
    assert cam <= 0.5 * tc.GRADIENT_TOLERANCE and lam >= 2 * tc.GRADIENT_TOLERANCE


def test_radius_case_ends_on_the_minimum_radius():
    so, st, sn, x = solved("radius")
    n = so.num_iterations
    assert so.termination == tc.RADIUS and sn["termination_code"] == tc.RADIUS
    assert n >= 121                                        # 1e4 x 2^-k < 1e-32 needs k >= 120 rejections
    assert so.radius[n - 1] < 2.3e-32                      # the radius the last record used: one halving above the threshold at most
    assert max(so.rho[i] for i in range(1, n) if not so.step_ok[i]) <= 0.0
    print("radius: %d records, last stored radius %.3e, final cost %.12e" % (n, so.radius[n - 1], so.final_cost))


def test_time_offset_window_decision_is_clear_and_stable():
    """the ESTIMATE_TD window of the device test (np_oracle only: the C oracle has no ProjectionTdFactor)"""
    w = tc.td_window()
    x, sn = NO.solve(NO.Problem(w), 100, False)
    deciding, least = tc.check_margins(sn)
    tc.check_trace_rules(tc.np_summary(sn), len(sn["iterations"]))
    print("time offset window ends on %s after %d records: deciding quantity %.3g x its threshold, smallest earlier quantity %.3g x" %
          (sn["termination"], len(sn["iterations"]), deciding, least))
    x2, s2 = NO.solve(NO.Problem(tc.perturbed(w, 0)), 100, False)
    assert tc.np_trace_of(s2) == tc.np_trace_of(sn)


def test_every_termination_code_is_covered():
    """0 .. 4 each by a case with the conditions above; 1 both at entry and after an accepted step"""
    assert sorted(set(t for t, _ in tc.EXPECTED.values())) == [0, 1, 2, 3, 4]
    assert tc.EXPECTED["gradient_at_entry"] == (tc.GRADIENT, 1) and tc.EXPECTED["gradient"][1] > 1
