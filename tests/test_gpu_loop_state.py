"""The trust-region loop of the solve kernel keeps the doubles it carries from one phase call to the next (cost, radius, mu, the dogleg's
dot products, the step's coefficients, ...) in one small block of LDS that all wavefronts of the workgroup share (tcv_solve.hip LoopState).
What a misplaced or stale slot of that block would break, on the cases of tests/termination_cases.py (tests/test_gpu_termination.py holds
every termination path against the oracles; nothing here needs an oracle):

1. nothing leaks from one window to the next one the same workgroup solves: batches of 2 x CUs + 16 windows (some workgroups take two in
   sequence) with a long run (`radius`: the radius halved down to 1e-32), a run through accepted and rejected steps and all dogleg cases
   (`function`) and a filler that ends before the first iteration (`gradient_at_entry`), in two orders and with the convergence tests
   off and on, and with the two long runs back to back in the same workgroups (the second group at grid .. grid + 7): every copy of a
   case gives the same trace and the same states, bit for bit;
2. every path that carries state across a call: the summary against the loop's own arithmetic (termination_cases.check_trace_rules: rho,
   radius, mu record by record, so a stale slot shows at the record where it is read) -- every case with the convergence tests on in a
   batch larger than the CU count (chain instance), an ESTIMATE_TD window (the instance with ProjectionTdFactor), a lone window on
   1 + H workgroups (the cooperative master), a window of the benchmark with 8 fixed iterations, a run the solver-time budget stops,
   a run with more records than the summary stores, a run of invalid steps (mu raised tenfold each time, the one path off mu = 1e-8
   a finite window reaches);
3. the cooperative instance and the chain instance give the same bits on one ESTIMATE_TD window, trace and states.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import synth
import termination_cases as tc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev"))
import fuzz_solve as fz      # noqa: E402

pytestmark = pytest.mark.gpu
STORED = 64                  # TCV_MAX_TRACE
TRACE = ("cost", "radius", "mu", "rho", "step_norm", "model_cost_change", "cost_candidate", "dogleg_case", "step_ok")


def compute_units(gpu):
    out = (C.c_double * 4)()
    gpu.check(gpu.lib().tcv_microbench_fp64(out))
    assert out[2] >= 1
    return int(out[2])


def trace_bits(s):
    """the trace of a device summary as bytes: equal means bit for bit (a NaN included)"""
    return (s.num_iterations, s.termination) + tuple(bytes(getattr(s, f)) for f in TRACE)


def state_bits(W):
    return tuple((k, np.ascontiguousarray(v).tobytes()) for k, v in sorted(W.states().items()))


def run(gpu, names, iters, fixed, **kw):
    """one batch of the named cases, solved once: (windows, batch, summaries)"""
    cs = tc.cases()
    Ws = [gpu.Window(cs[n][0], estimate_extrinsic=not cs[n][2]) for n in names]
    b = gpu.Batch(Ws)
    b.solve(gpu.default_options(iters, fixed, True, 256, True, **kw)); b.synchronize(); b.download_states()
    return Ws, b, b.summaries()


def test_no_state_leaks_from_one_window_to_the_next_of_a_workgroup(gpu):
    """A workgroup takes windows slot, slot + grid, slot + 2 grid, ...  Two batches put `radius` first and `function` last (and the other
    way round) with the filler between them; two more put the second group at grid .. grid + 7, so that workgroups 0 .. 7 solve a
    `radius` run and then a `function` run back to back (and the other way round): the filler ends before it reads a slot back."""
    n = 2 * compute_units(gpu) + 16
    fill = "gradient_at_entry"

    def ends(first, last):
        return [first] * 8 + [fill] * (n - 16) + [last] * 8

    def back_to_back(first, second, grid):
        names = [fill] * n
        names[0:8] = [first] * 8
        names[grid:grid + 8] = [second] * 8
        return names
    for iters, fixed in ((130, True), (130, False)):      # (`radius` needs the tests off to get to the minimum radius, the other two need them on)
        seen = {}
        grid = None

        def solve_and_compare(names):
            Ws, b, s = run(gpu, names, iters, fixed)
            st = b.plan_stats()
            assert st["layout"] == "chain" and st["grid"] < n, st      # some workgroups solve two windows in sequence
            for k, name in enumerate(names):
                got = (trace_bits(s[k]), state_bits(Ws[k]))
                want = seen.setdefault(name, got)
                assert got[0] == want[0], (name, k, fixed, "trace")
                assert got[1] == want[1], (name, k, fixed, "states")
            return st["grid"]
        for names in (ends("radius", "function"), ends("function", "radius")):
            g = solve_and_compare(names)
            assert grid in (None, g)
            grid = g
        assert 8 <= grid and grid + 8 <= n
        for first, second in (("radius", "function"), ("function", "radius")):
            names = back_to_back(first, second, grid)
            assert all(names[i] == first and names[i + grid] == second for i in range(8))      # window i + grid follows window i in workgroup i
            assert solve_and_compare(names) == grid
        rad, fun, gra = (seen[c][0] for c in ("radius", "function", "gradient_at_entry"))
        print("tests %s, grid %d of %d windows: radius %d records, termination %d; function %d, %d; gradient_at_entry %d, %d" %
              (("off", "on")[not fixed], grid, n, rad[0], rad[1], fun[0], fun[1], gra[0], gra[1]))
        if fixed:
            assert (rad[1], rad[0]) == tc.EXPECTED["radius"]
        else:
            assert (fun[1], fun[0]) == tc.EXPECTED["function"] and (gra[1], gra[0]) == tc.EXPECTED["gradient_at_entry"]


def invalid_step_window():
    """the prior-only window of termination_cases with J0 = 0: the cost is |r0|^2 / 2 whatever the states, gradient and Gauss-Newton
    step are exactly zero, model_cost_change is 0 and every step invalid -- mu goes up tenfold each time until the fifth ends the run"""
    w = dict(tc.prior_only_window())
    p = dict(w["prior"])
    p["J0"] = np.zeros_like(np.asarray(p["J0"], dtype=float))
    w["prior"] = p
    return w


def test_invalid_steps_raise_mu_alike_in_every_wavefront_and_window(gpu):
    """The mu * 10 of an invalid step reads and rewrites its slot with no phase call in between (the barrier in front of the store is what
    keeps a fast wavefront from raising it twice for a slow one): 8 fixed iterations, more windows than workgroups, the trace against the
    sequence itself and bit for bit across the copies.  (No finite window reaches the other mu * 10, behind a failed factorisation:
    J'J + mu D^2 is positive definite, and the 600 fuzz structures and every case of termination_cases stay at mu = 1e-8.)"""
    n = 2 * compute_units(gpu) + 16
    w = invalid_step_window()
    Ws, b, s = fz.gpu_run(w, False, copies=n, iters=8, fixed=True)
    assert b.plan_stats()["layout"] == "chain" and b.plan_stats()["grid"] < n
    mus = [1e-8]
    for _ in range(4):
        mus.append(mus[-1] * 10.0)
    print("invalid steps: %d records, termination %d, mu %s" % (s[0].num_iterations, s[0].termination, [s[0].mu[i] for i in range(1, 6)]))
    for k in (0, n - 1):
        assert (s[k].termination, s[k].num_iterations) == (tc.FAILURE, 6)
        assert [s[k].mu[i] for i in range(1, 6)] == mus
        assert [s[k].dogleg_case[i] for i in range(1, 6)] == [-1] * 5 and [s[k].step_ok[i] for i in range(1, 6)] == [0] * 5
        assert [s[k].radius[i] for i in range(1, 6)] == [1e4] * 5
        assert all(s[k].cost[i] == s[k].initial_cost for i in range(6)) and s[k].final_cost == s[k].initial_cost > 0
    first = (trace_bits(s[0]), state_bits(Ws[0]))
    for k in range(1, n):
        assert (trace_bits(s[k]), state_bits(Ws[k])) == first, k


@pytest.mark.parametrize("name", [n for n in tc.EXPECTED if n != "radius"])
def test_chain_instance_trace_follows_the_loops_arithmetic(gpu, name):
    w_hip, w_orc, exc, iters, fixed = tc.cases()[name]
    assert not fixed
    copies = compute_units(gpu) + 1
    Ws, b, s = fz.gpu_run(w_hip, exc, copies=copies, iters=iters, fixed=fixed)
    assert b.plan_stats()["layout"] == "chain" and b.cooperative()["helpers"] == 0
    want_t, want_n = tc.EXPECTED[name]
    for k in (0, copies - 1):
        print("%s window %d: %d records, termination %d" % (name, k, s[k].num_iterations, s[k].termination))
        assert (s[k].termination, s[k].num_iterations) == (want_t, want_n)
        tc.check_trace_rules(s[k], min(s[k].num_iterations, STORED))
    assert trace_bits(s[0]) == trace_bits(s[copies - 1])


def test_trace_with_more_records_than_the_summary_stores(gpu):
    w_hip, w_orc, exc, iters, fixed = tc.cases()["long_trace_seed0"]
    assert iters > STORED
    copies = compute_units(gpu) + 1
    Ws, b, s = fz.gpu_run(w_hip, exc, copies=copies, iters=iters, fixed=fixed)
    k = copies - 1
    assert s[k].num_iterations == iters + 1 and s[k].termination == tc.NO_CONVERGENCE
    tc.check_trace_rules(s[k], STORED)
    assert s[k].final_cost < s[k].cost[STORED - 1]      # the loop went on behind the stored records, with the state it carried there


def test_time_offset_instance_trace_follows_the_loops_arithmetic(gpu):
    copies = compute_units(gpu) + 1
    Ws, b, s = fz.gpu_run(tc.td_window(), False, copies=copies, iters=100, fixed=False)
    assert b.plan_stats()["layout"] == "chain" and b.cooperative()["helpers"] == 0
    k = copies - 1
    assert s[k].termination in (tc.GRADIENT, tc.PARAMETER, tc.FUNCTION) and s[k].num_iterations > 2
    tc.check_trace_rules(s[k], min(s[k].num_iterations, STORED))
    assert trace_bits(s[0]) == trace_bits(s[k])


def test_cooperative_master_trace_follows_the_loops_arithmetic(gpu):
    w_hip, w_orc, exc, iters, fixed = tc.cases()["parameter_main"]
    Ws, b, s = fz.gpu_run(w_hip, exc, copies=1, iters=iters, fixed=fixed, workgroups_per_window=0)
    co = b.cooperative()
    assert co["helpers"] > 0 and co["last_solve_workgroups"] == 1 + co["helpers"], co
    assert (s[0].termination, s[0].num_iterations) == tc.EXPECTED["parameter_main"]
    tc.check_trace_rules(s[0], min(s[0].num_iterations, STORED))


def test_benchmark_window_with_fixed_iterations(gpu):
    import bench
    batch, wins, keep = bench.build_batches(gpu, synth, 0, 4)
    batch.solve(gpu.default_options(bench.SOLVER_ITERATIONS, True)); batch.synchronize()
    s = batch.summaries()
    for k in range(4):
        assert s[k].num_iterations == bench.SOLVER_ITERATIONS + 1 and s[k].termination == tc.NO_CONVERGENCE
        tc.check_trace_rules(s[k], s[k].num_iterations)


def test_run_stopped_by_the_solver_time_budget(gpu):
    """The budget ends the run between two iterations, which one depends on the clock: gated on what does not -- NO_CONVERGENCE, fewer
    records than the free run, and the records that are there follow the loop's arithmetic up to the final cost."""
    w_hip, w_orc, exc, iters, fixed = tc.cases()["parameter_main"]

    def solve(budget):
        W = gpu.Window(w_hip, estimate_extrinsic=not exc); b = gpu.Batch([W])
        o = gpu.default_options(iters, False, True, 256, True, 1); o.max_solver_time_in_seconds = budget
        b.solve(o); b.synchronize()
        return b.summaries()[0]
    free = solve(0.0)
    assert (free.termination, free.num_iterations) == tc.EXPECTED["parameter_main"]
    s = solve(6e-4)      # (one iteration of a lone window on one workgroup takes ~0.3 ms: the budget is over after the first few)
    print("budget 0.6 ms: %d records, termination %d" % (s.num_iterations, s.termination))
    assert s.termination == tc.NO_CONVERGENCE and 1 <= s.num_iterations < free.num_iterations
    n = s.num_iterations
    tc.check_trace_rules(s, n)
    for f in TRACE:      # the records it has are the free run's
        assert list(getattr(s, f))[:n] == list(getattr(free, f))[:n], f


@pytest.mark.parametrize("iters,fixed", [(8, True), (100, False)])
def test_cooperative_and_chain_instance_give_the_same_bits_on_a_time_offset_window(gpu, iters, fixed):
    w = synth.with_time_offset(synth.window_at(synth.make_windows(41, 1), 0), 41, TR=0.02)
    res = {}
    for wg in (0, 1):
        W = gpu.Window(w); b = gpu.Batch([W])
        assert b.plan_stats()["layout"] == "chain"
        b.solve(gpu.default_options(iters, fixed, workgroups_per_window=wg)); b.synchronize(); b.download_states()
        res[wg] = (b.cooperative(), trace_bits(b.summaries()[0]), state_bits(W))
    co = res[0][0]
    assert co["helpers"] >= 2 and co["last_solve_workgroups"] == 1 + co["helpers"] and res[1][0]["last_solve_workgroups"] == 1, co
    assert res[0][1] == res[1][1]
    assert res[0][2] == res[1][2]
