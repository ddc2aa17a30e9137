"""Every termination path of the fused solve loop (tc-viml_amd/csrc/tcv_solve.hip solve_kernel: the gradient test before the first iteration and
after an accepted step, the parameter and function tolerances, the iteration limit past TCV_MAX_TRACE = 64 records, the minimum radius)
against the C oracle, on the cases of tests/termination_cases.py -- windows on which both oracles end where the case says with the deciding
quantity <= 0.5 x its threshold and everything tested before it >= 2 x, and whose oracle trace does not move under 1e-13 state noise
(tests/test_termination_cpu.py asserts that without a device).  Each case runs in the settings of tests/dev/fuzz_solve.py -- lone (a batch
of one: cooperative where the window gets helpers), single (TCV_COOP_H=0), packed (257 copies: two workgroups per CU, 80 KiB of LDS each),
dense (solver variant 1) --, parameter_main also without MFMA and with 512 threads, parameter_main and long_trace_seed17 explicitly in
cooperative mode (helpers > 0 asserted).

Gates against the oracle: num_iterations and termination equal (beyond 64 records too); step_ok and dogleg_case equal and the costs within
TOL = 1e-6 over min(n, 64) records; final cost within 1e-6 (where the oracle ends below 1e-12: below 1e-12); states within 1e-6 as a whole
and per parameter family; check_trace_rules (the loop's own arithmetic, no oracle) on the device summary.  `radius` is gated on what is well
posed there (see test_minimum_radius).  One ESTIMATE_TD window runs (100, to convergence) against np_oracle.solve.

Measured on an MI355X (profiles/termination_parity.txt; test_zz_report prints the figures per case and setting): every case in every
setting ends on the oracle's record count and termination with the oracle's accepts and dogleg cases.  Worst figures over the settings:
costs over the records 4.9e-10 (gradient_at_entry: a cost of 2e-18), otherwise 1.3e-10; final cost 1.5e-9 (long_trace_seed0); states per
family 9.99e-7 (parameter_small, extrinsic translation: nine frames, one landmark -- the two ORACLES are 5.9e-6 apart there), then
6.2e-7 (long_trace_seed0), 4.9e-7 (parameter_small2), 3.0e-7 (parameter_main); the ESTIMATE_TD window ends on the function tolerance after
22 records, final cost 1.3e-9, states 3.7e-8.  radius: 124 records (dense: 125), final cost 1.7e-9 from the oracle's with the oracle's own
spread at 4.2e-10, no rejected step with rho > 0.  Helpers in the lone setting: parameter_main 2, long_trace_seed17 7, the others none.
The same file records which of these tests fail on four deliberately wrong loops (scratch builds)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import np_oracle as NO
import orc
import termination_cases as tc
from test_gpu_solve import check_states_by_family
from util import fmt_families, rel, rel_by_family, state_families

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev"))
import fuzz_solve as fz      # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
STORED = 64                  # TCV_MAX_TRACE
REPORT = {}                  # (case, setting) -> figures, printed by test_zz_report
NOTES = []
SETTINGS = {"lone": dict(copies=1), "single": dict(copies=1, coop_off=True), "packed": dict(copies=257), "dense": dict(copies=1, dense=True)}
EXTRA = {"no_mfma": dict(copies=1, mfma=False), "threads512": dict(copies=1, threads=512)}
_ORACLE = {}


def oracle(name):
    """(C summary, C states) of a case, solved once"""
    if name not in _ORACLE:
        w_hip, w_orc, exc, iters, fixed = tc.cases()[name]
        O = orc.Window(w_orc, ex_constant=exc)
        _ORACLE[name] = (O.solve(iters, fixed), O.states())
    return _ORACLE[name]


def device(name, **kw):
    w_hip, w_orc, exc, iters, fixed = tc.cases()[name]
    return fz.gpu_run(w_hip, exc, iters=iters, fixed=fixed, **kw)


def fields(s):
    """every field of a device summary (all 64 entries of the arrays: a fresh batch's summaries start zeroed)"""
    return [getattr(s, f) if not hasattr(getattr(s, f), "__len__") else list(getattr(s, f)) for f, _ in type(s)._fields_]


def check_against(s, sg, so, st, tag):
    """the gates of the module docstring on one device summary `s` with states `sg` against the oracle's (so, st); so: a C summary or
    termination_cases.np_summary"""
    fig = REPORT.setdefault(tag, {})
    fig["records"], fig["termination"] = s.num_iterations, s.termination
    print("%s: device %d records, termination %d; oracle %d, %d" % (tag, s.num_iterations, s.termination, so.num_iterations, so.termination))
    assert (s.num_iterations, s.termination) == (so.num_iterations, so.termination), tag
    n = min(so.num_iterations, STORED)
    assert [s.step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)], tag
    assert [s.dogleg_case[i] for i in range(1, n)] == [so.dogleg_case[i] for i in range(1, n)], tag
    fig["costs"] = rel([s.cost[i] for i in range(n)], [so.cost[i] for i in range(n)])
    if so.final_cost < 1e-12:      # (a zero-residual fit: the last digits of a cost of 1e-20 are rounding noise)
        fig["final cost (absolute, oracle below 1e-12)"] = s.final_cost
    else:
        fig["final cost"] = abs(s.final_cost - so.final_cost) / so.final_cost
    byf = rel_by_family(state_families(sg), state_families(st))
    fig["state family"] = max(byf.values()) if byf else 0.0
    print("   costs %.2e  final cost %.6e vs %.6e  states %s" % (fig["costs"], s.final_cost, so.final_cost, fmt_families(byf)))
    assert fig["costs"] < TOL, tag
    if so.final_cost < 1e-12:
        assert s.final_cost < 1e-12, tag
    else:
        assert fig["final cost"] < TOL, tag
    for key in ("pose", "sb", "ex", "lam", "td"):
        if st.get(key) is not None and np.asarray(st[key]).size:
            assert rel(sg[key], st[key]) < TOL, (tag, key)
    check_states_by_family(sg, st, TOL, tag)
    tc.check_trace_rules(s, n)


CASES = [n for n in tc.EXPECTED if n != "radius"]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", CASES)
def test_case_ends_like_the_oracle(gpu, name, setting):
    so, st = oracle(name)
    assert (so.termination, so.num_iterations) == tc.EXPECTED[name]
    Ws, b, s = device(name, **SETTINGS[setting])
    k = len(Ws) - 1
    check_against(s[k], Ws[k].states(), so, st, (name, setting))
    if setting == "packed":      # the same window gives the same summary wherever it runs in the batch
        first = fields(s[0])
        assert all(fields(s[j]) == first for j in range(1, len(Ws))), name
    if setting == "lone":
        REPORT[(name, setting)]["helpers"] = b.cooperative()["helpers"]


@pytest.mark.parametrize("setting", list(EXTRA))
def test_parameter_tolerance_without_mfma_and_with_512_threads(gpu, setting):
    so, st = oracle("parameter_main")
    Ws, b, s = device("parameter_main", **EXTRA[setting])
    check_against(s[0], Ws[0].states(), so, st, ("parameter_main", setting))


@pytest.mark.parametrize("name", ["parameter_main", "long_trace_seed17"])
def test_cooperative_mode_reads_the_helpers_gradient_and_norms(gpu, name):
    """1 + H workgroups per window: the landmark part of the gradient (grad_max) and of the scaled vectors is written by the helpers; the
    master's tests read it.  A window that gets no helpers fails here instead of passing as a second `single` run."""
    so, st = oracle(name)
    Ws, b, s = device(name, copies=1, workgroups_per_window=0)
    co = b.cooperative()
    if not co["helpers"] > 0:
        NOTES.append("%s got no helper workgroups: the cooperative setting did not run" % name)
    assert co["helpers"] > 0 and co["last_solve_workgroups"] == 1 + co["helpers"], co
    check_against(s[0], Ws[0].states(), so, st, (name, "cooperative, %d helpers" % co["helpers"]))
    W1, b1, s1 = device(name, copies=1, workgroups_per_window=1)      # the same plan on one workgroup: the same bits
    assert b1.cooperative()["last_solve_workgroups"] == 1
    assert fields(s[0]) == fields(s1[0])


@pytest.mark.parametrize("name", tc.LONG_TRACE)
def test_trace_beyond_the_stored_records_keeps_its_layout(gpu, name):
    """101 records in a summary that stores 64: entries 0 .. 63 are the first 64 records, num_iterations is 101, final_cost and termination
    are those of record 100, and nothing is written behind the arrays -- the next window's summary (a short trace of another window, and
    the 0xA5 pattern behind the last one) is intact."""
    so, st = oracle(name)
    others = ["parameter_small2", "gradient_at_entry"]
    names = [name, others[0], name, others[1]]
    wins = [tc.cases()[n] for n in names]
    Ws = [gpu.Window(w[0], estimate_extrinsic=not w[2]) for w in wins]
    b = gpu.Batch(Ws)
    b.solve(gpu.default_options(100, False, True, 256, True)); b.synchronize(); b.download_states()
    size = C.sizeof(gpu.SolverSummary)
    arr = (gpu.SolverSummary * (len(Ws) + 1))()
    C.memset(arr, 0xA5, size * (len(Ws) + 1))
    gpu.check(gpu.lib().tcv_batch_get_summaries(b.h, arr, len(Ws)))
    assert C.string_at(C.addressof(arr[len(Ws)]), size) == b"\xa5" * size
    for k, n in enumerate(names):
        o, ost = oracle(n)
        check_against(arr[k], Ws[k].states(), o, ost, (n, "mixed batch, window %d" % k))
    for k in (0, 2):
        s = arr[k]
        assert s.num_iterations == 101 and s.termination == tc.NO_CONVERGENCE
        assert abs(s.cost[63] - so.cost[63]) < TOL * so.cost[63] and abs(s.final_cost - so.cost[100]) < TOL * so.cost[100]
        assert so.cost[100] < so.cost[63] and s.final_cost < s.cost[63]      # the final cost is not the last STORED record's
    assert fields(arr[0]) == fields(arr[2])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_minimum_radius(gpu, setting):
    """130 fixed iterations at a state the trust region cannot leave: the radius is halved until it is below 1e-32 (termination 4).  From
    record ~50 on the numerator of rho is the rounding of two evaluations of the same cost, so accept / reject is not compared with the
    oracle (its own trace moves in 3 of 3 draws of 1e-13 noise); gated on what is well posed: termination 4, at least 121 records
    (1e4 x 2^-k < 1e-32 needs k >= 120 halvings), the loop's own arithmetic over the 64 stored records, no rejected step with rho > 0 (the
    candidate equals the state or lies uphill), and the final cost within 30 x the C oracle's own spread under the three 1e-13 draws."""
    so, st = oracle("radius")
    if "radius spread" not in _ORACLE:
        w_hip, w_orc, exc, iters, fixed = tc.cases()["radius"]
        _ORACLE["radius spread"] = max(abs(orc.Window(tc.perturbed(w_orc, rep), ex_constant=exc).solve(iters, fixed).final_cost - so.final_cost) / so.final_cost
                                       for rep in range(3))
    spread = _ORACLE["radius spread"]
    Ws, b, s = device("radius", **SETTINGS[setting])
    k = len(Ws) - 1
    d = abs(s[k].final_cost - so.final_cost) / so.final_cost
    worst_rejected = max(s[k].rho[i] for i in range(1, STORED) if not s[k].step_ok[i])
    REPORT[("radius", setting)] = {"records": s[k].num_iterations, "termination": s[k].termination, "final cost": d, "oracle's own spread": spread,
                                   "largest rho of a rejected step": worst_rejected}
    print("radius %s: %d records (oracle %d), termination %d, final cost %.3e from the oracle's, the oracle's own spread %.3e, largest rejected rho %.3e" %
          (setting, s[k].num_iterations, so.num_iterations, s[k].termination, d, spread, worst_rejected))
    assert s[k].termination == tc.RADIUS and s[k].num_iterations >= 121
    tc.check_trace_rules(s[k], STORED)
    assert worst_rejected <= 0.0
    assert d <= 30 * spread, (d, spread)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_time_offset_window_to_convergence(gpu, setting):
    """every point factor a ProjectionTdFactor: the td block is part of |x| and |x+ - x| and of the gradient"""
    if "td" not in _ORACLE:
        w = tc.td_window()
        x, sn = NO.solve(NO.Problem(w), 100, False)
        NOTES.append("the ESTIMATE_TD window ends on %s after %d records" % (sn["termination"], len(sn["iterations"])))
        _ORACLE["td"] = (w, x, tc.np_summary(sn))
    w, x, so = _ORACLE["td"]
    Ws, b, s = fz.gpu_run(w, False, iters=100, fixed=False, **SETTINGS[setting])
    k = len(Ws) - 1
    check_against(s[k], Ws[k].states(), so, x, ("time offset window", setting))


def test_zz_report():
    for (name, setting), fig in REPORT.items():
        print("%-20s %-28s %s" % (name, setting, "  ".join("%s %s" % (k, ("%.2e" % v) if isinstance(v, float) else v) for k, v in fig.items())))
    for n in NOTES:
        print("note:", n)
