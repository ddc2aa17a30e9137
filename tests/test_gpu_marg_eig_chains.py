"""The eigen-solver of A' (csrc/tcv_marg.hip sym_eig_tridiag) after its dependent chains were shortened: two lanes per eigenvector in the
twisted factorisation (the backward pivots pass through the workgroup's global scratch), a Gram-Schmidt whose columns stay in registers
and whose cluster boundaries come from a ballot, the next Householder step's scalars formed inside the update of the step before, the
Gershgorin bounds by one lane per row, the self-check's loads in batches.  The arithmetic and every order of summation are those of the
one-lane forms (profiles/marg_eig_chains.txt: bit-identical priors against the parent commit); here the paths are run on the windows
that reach them, at bit-identical states against the oracles, in both launch shapes, twice and in reversed window order.

Cases (the property each one is there for is asserted on the ORACLE's A' before anything of the device is looked at):
  bench      the 16 benchmark-shaped windows of bench.build_batches(.., 100000, 16), at the states the C oracle's solve ends in: n = 75
             with a rank-40 GPU-made prior among the factors.  Every A' is rank deficient (null cluster, zero columns, the lanes that skip
             the factorisation).  The windows without a group of >= 3 retained eigenvalues within 1e-10 |T| (the Gram-Schmidt path with
             more than one earlier column per vector) cannot fail that path and are listed in the output; at least one must have one.
             (At a window's initial states b' is a small difference of large terms, and the NumPy oracle's own b' is 1e-6 .. 2e-5 from a
             50-digit Schur step, tests/test_pins_cpu.py: further than its gate.  Hence the solved states, here and below.)
  ragged     sub-windows without a prior, at the states the C oracle's solve ends in:
               two_frames  first 2 frames, n = 21: one wavefront, one term per lane in the Gram-Schmidt dots
               n63, n69    first 9 and 10 frames: the two sides of 64 (second term per lane, second wavefront of the row-wise phases);
                           each must have a group of >= 3 close retained eigenvalues
             two_frames IS NOT GATEABLE AGAINST THE ORACLES: its Amm has eigenvalues at the eps threshold of the pseudo-inverse and the C
             and the NumPy oracle are 9e-5 apart in A' on it (2e-5 .. 2e-3 on every two-frame window looked at, seeds 400 and
             7100 .. 7112), more than the two gates together; the test asserts that distance instead, prints the device's figures, and keeps every other
             check of the case.  The seeds are the ones on which the two oracles are closest to each other (n63 5e-8 / 4e-10, n69
             7e-8 / 2e-9 in A' / b') and, for two_frames, on which the part of A', b' that the thresholding removes is smallest.
  td         an ESTIMATE_TD window at the states the NumPy oracle's solve ends in, as in tests/test_gpu_td.py: n = 76, the largest n a
             10-keyframe window reaches.  NumPy oracle only: the C oracle cannot form a td window.
  solved     the 16 benchmark windows again, marginalised behind the device's own solve and gauge fix as bench.py does it: the heavily
             clustered small eigenvalues of a second-generation prior, where the Gram-Schmidt step has most of its work.

Gates, all fixed figures of existing tests:
  tests/test_gpu_marg.py, launch shapes and TCV_MARG_EIG_FLAGS: A', b' bit for bit between the shapes; J0'J0 = A' to 2e-6, J0'r0 = b' to 5e-5;
      J0'J0 between the shapes to 1e-9, J0'r0 between the shapes to 1e-7 |b'|; the same number of zero rows, at least 4, leading.
  tests/test_gpu_marg.py, at bit-identical states: A', J0'J0 against the C oracle's A' to 2e-6, b' to 1e-8.
  tests/test_gpu_td.py, the existing comparison of a device-made MARGIN_OLD prior with the NumPy oracle: A', J0'J0 to 1e-5, b' to 1e-6
      against the NumPy oracle, for every case (its LAPACK eigh of the graded Amm is accurate in the absolute sense only; the C oracle's
      cyclic Jacobi in the relative sense, tests/test_pins_cpu.py).
  tests/test_gpu_bench_shape.py, each side behind its own solve (`solved`): A' to 4e-6, b' to 3e-6 against the C oracle.
Diagnostics (TCV_DEBUG dump of MARG_DIAG_EIG_CHECK):
  dev    below the kernel's own 1e-7;
  trace  that of the device's A' to the eleven digits the dump prints;
  sum    of the retained eigenvalues: LAPACK's, of the device's A', to the kernel's own 1e-9 n |T| (its round-2 gate of sum against trace);
         LAPACK's, of the oracle's A' (gateable cases), to n times the A' gate times |A'| (Weyl: no eigenvalue moves further than |dA|);
         an eigenvalue that sits at the threshold may be counted on one side only: n * 1e-8 on both;
  |T|    the Gershgorin bound of the tridiagonal form, which is similar to A' and whose entries are bounded by the spectral radius rho:
         rho <= |T| <= 3 rho, no tolerance but the four digits printed.
Every figure is printed before the case asserts."""
import re

import numpy as np
import pytest

import np_oracle as NO
import orc
import synth
from util import fro, sub_window

pytestmark = pytest.mark.gpu

NUMPY_GATES = (1e-5, 1e-6)          # tests/test_gpu_td.py
RAGGED = (("two_frames", 7109, 2, 21), ("n63", 7107, 9, 63), ("n69", 7107, 10, 69))
NOT_GATEABLE = ("two_frames",)

_CACHE = {}


def _cluster(lam):
    """largest group of retained eigenvalues whose neighbours are within 1e-10 of the spectral radius"""
    T = max(abs(lam[0]), abs(lam[-1]))
    ret = lam[lam > 1e-8]
    best, i = 0, 0
    while i < len(ret):
        j = i
        while j + 1 < len(ret) and ret[j + 1] - ret[j] <= 1e-10 * T:
            j += 1
        best = max(best, j - i + 1); i = j + 1
    return best


def _spectrum(A):
    return np.linalg.eigvalsh(0.5 * (A + A.T))


def _oracles(w, numpy_only=False):
    """A', b' of the oracles at the window's own states (the C oracle first), their distance from each other, the spectrum of the first one's A'"""
    P = NO.Problem(w)
    pn, dn = NO.marginalize_old(P, P.x0())
    ref, dist = [dn], None
    if not numpy_only:
        pc, dc = orc.Window(w).marginalize_old()
        ref = [dc, dn]
        dist = (fro(dn["A_schur"], dc["A_schur"]), fro(dn["b_schur"], dc["b_schur"]))
    return dict(ref=ref, dist=dist, lam=_spectrum(ref[0]["A_schur"]), n=pn["n"], m=pn["m"])


def _at_c_oracle_solution(w):
    O = orc.Window(w); O.solve(8, True); st = O.states()
    return dict(w, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])


def bench_windows(gpu):
    """the 16 benchmark-shaped windows at their initial states, each with its GPU-made prior"""
    if "bench_initial" not in _CACHE:
        import bench
        _CACHE["bench_initial"] = bench.build_batches(gpu, synth, 100000, 16)[1]
    return _CACHE["bench_initial"]


def cases(gpu, group):
    """(names, windows, oracles, (A' gate, b' gate) for the C oracle), built once per session"""
    if group in _CACHE:
        return _CACHE[group]
    if group == "bench":
        names = ["bench%d" % k for k in range(16)]
        wins = [_at_c_oracle_solution(w) for w in bench_windows(gpu)]
        gates = (2e-6, 1e-8)
    elif group == "ragged":
        names = [c[0] for c in RAGGED]
        wins = [_at_c_oracle_solution(sub_window(synth.window_at(synth.make_windows(seed, 1, frame_shift=-1), 0), f)) for _, seed, f, _ in RAGGED]
        gates = (2e-6, 1e-8)
    else:
        w = synth.with_time_offset(synth.window_at(synth.make_windows(23, 1), 0), 23)
        x, _ = NO.solve(NO.Problem(w), 8, True)
        names = ["td"]
        wins = [dict(w, pose=x["pose"], speedbias=x["sb"], ex_pose=x["ex"], lam=x["lam"], td=float(x["td"][0]))]
        gates = NUMPY_GATES
    orcs = [_oracles(w, numpy_only=(group == "td")) for w in wins]
    _CACHE[group] = (names, wins, orcs, gates)
    return _CACHE[group]


def batch_of(gpu, wins, order=None):
    order = list(range(len(wins))) if order is None else order
    W = [gpu.Window(wins[k]) for k in order]
    MW = [gpu.margin_old_window(wins[k]) for k in order]
    M = [gpu.Window(mw, share=W[i]) for i, mw in enumerate(MW)]
    drops = [gpu.margin_old_drops(W[i], MW[i]) for i in range(len(order))]
    return gpu.Batch(W, M, drops), {k: i for i, k in enumerate(order)}, (W, M)


def marginalise(gpu, wins, order=None, solve=False):
    """one batch, marginalised at the windows' own (host) states, or behind the device's solve and gauge fix as bench.py runs it:
    (batch, position of every window of `wins` in it, what has to stay alive)"""
    b, pos, hold = batch_of(gpu, wins, order)
    if solve:
        import bench
        b.solve(gpu.default_options(bench.SOLVER_ITERATIONS, True)); b.gauge_fix()
    b.marginalize(); b.synchronize()
    return b, pos, hold


def check_properties(group, names, orcs, gates):
    ns = [o["n"] for o in orcs]
    ranks = [int((o["lam"] > 1e-8).sum()) for o in orcs]
    groups = [_cluster(o["lam"]) for o in orcs]
    notes = ["%s: n %s rank %s largest group of retained eigenvalues within 1e-10 |T| %s" % (group, ns, ranks, groups)]
    assert all(r < n for r, n in zip(ranks, ns)), (ranks, ns)                  # a null cluster in every window
    if group in ("bench", "solved"):
        assert ns == [75] * 16
        without = [k for k, g in enumerate(groups) if g < 3]
        notes.append("%s windows without a group of >= 3 close retained eigenvalues (they cannot fail the Gram-Schmidt path): %s" % (group, without))
        assert len(without) < 16
    elif group == "ragged":
        assert ns == [c[3] for c in RAGGED] == [21, 63, 69]                    # one wavefront; just below and just above 64
        assert groups[1] >= 3 and groups[2] >= 3, groups                       # Gram-Schmidt with the second term per lane
        notes.append("two_frames, n63, n69: the C and the NumPy oracle are apart by %s" % ", ".join("A' %.1e b' %.1e" % o["dist"] for o in orcs))
        for name, o in zip(names, orcs):
            if name in NOT_GATEABLE:                                           # ... because its two oracles are further apart than the gate
                assert o["dist"][0] > gates[0] + NUMPY_GATES[0], o["dist"]      # no A' is within its gate of both
                notes.append("%s cannot be gated against the oracles: they are %.1e apart in A', the gates are %.0e and %.0e" % (name, o["dist"][0], gates[0], NUMPY_GATES[0]))
    else:
        assert ns == [76]
        notes.append("td: NumPy oracle only")
    return notes


@pytest.mark.parametrize("group", ["bench", "ragged", "td"])
@pytest.mark.parametrize("nt", ["256", "512"])
def test_eigen_solver_chains_vs_oracles_in_both_shapes(gpu, monkeypatch, capfd, nt, group):
    names, wins, orcs, (gA, gb) = cases(gpu, group)
    notes = check_properties(group, names, orcs, (gA, gb))      # (printed at the end: capfd swallows what is printed while it collects the TCV_DEBUG dump)
    fails = []

    def gate(ok, what):
        if not ok:
            fails.append(what)

    monkeypatch.setenv("TCV_MARG_NT", nt)
    b, pos, hold = marginalise(gpu, wins)
    assert list(b.marg_status()) == [0] * len(wins)                            # nobody on the Jacobi safety net, no sweep at its cap
    monkeypatch.setenv("TCV_MARG_NT", "512")
    b2, pos2, hold2 = marginalise(gpu, wins)
    try:
        for k, (name, o) in enumerate(zip(names, orcs)):
            capfd.readouterr()
            monkeypatch.setenv("TCV_DEBUG", "1")
            P = b.prior(k)
            monkeypatch.delenv("TCV_DEBUG")
            err = capfd.readouterr().err
            d = P.export(); As, bs = P.schur()
            d2 = b2.prior(k).export(); As2, bs2 = b2.prior(k).schur()
            assert (d["m"], d["n"]) == (o["m"], o["n"])
            # the comparisons of the launch-shape and TCV_MARG_EIG_FLAGS cases of test_gpu_marg.py
            JtJ, Jtr = d["J0"].T @ d["J0"], d["J0"].T @ d["r0"]
            JtJ2, Jtr2 = d2["J0"].T @ d2["J0"], d2["J0"].T @ d2["r0"]
            zero, zero2 = ~d["J0"].any(axis=1), ~d2["J0"].any(axis=1)
            notes.append("%s nt %s: J0'J0 vs A' %.2e  J0'r0 vs b' %.2e  between shapes J0'J0 %.2e J0'r0 %.2e |b'|  zero rows %d" % (
                name, nt, fro(JtJ, As), fro(Jtr, bs), fro(JtJ, JtJ2), np.linalg.norm(Jtr - Jtr2) / np.linalg.norm(bs), zero.sum()))
            gate(np.array_equal(As, As2) and np.array_equal(bs, bs2), name + ": A', b' differ between the shapes")
            gate(fro(JtJ, As) < 2e-6 and fro(Jtr, bs) < 5e-5, name + ": J0'J0 = A', J0'r0 = b'")
            gate(fro(JtJ, JtJ2) < 1e-9, name + ": J0'J0 between the shapes")
            gate(zero.sum() == zero2.sum() and zero.sum() >= 4 and not zero[zero.sum():].any(), name + ": zero rows")
            gate(np.linalg.norm(Jtr - Jtr2) <= 1e-7 * np.linalg.norm(bs), name + ": J0'r0 between the shapes")
            # against the oracles at bit-identical states
            for r, who in zip(o["ref"], ("C", "NumPy") if len(o["ref"]) == 2 else ("NumPy",)):
                tA, tb = (gA, gb) if who == "C" else NUMPY_GATES
                notes.append("    vs the %s oracle: A' %.2e  b' %.2e  J0'J0 %.2e%s" % (who, fro(As, r["A_schur"]), fro(bs, r["b_schur"]), fro(JtJ, r["A_schur"]),
                                                                                    "  (not gated)" if name in NOT_GATEABLE else ""))
                if name not in NOT_GATEABLE:
                    gate(fro(As, r["A_schur"]) < tA and fro(bs, r["b_schur"]) < tb, "%s: A', b' against the %s oracle" % (name, who))
                    gate(fro(JtJ, r["A_schur"]) < tA, "%s: J0'J0 against the %s oracle" % (name, who))
            # the self-check diagnostics of the eigen-solver
            mt = re.search(r"tridiag check: dev (\S+) sum\(lam\) (\S+) trace (\S+) \|T\| (\S+)", err)
            assert mt, err[-500:]
            dev, sl, tr, T = (float(x) for x in mt.groups())
            n, lam, lam_dev = o["n"], o["lam"], _spectrum(As)
            rho = max(abs(lam_dev[0]), abs(lam_dev[-1]))
            notes.append("    diagnostics: dev %.2e  sum lambda %.10e (LAPACK on the device's A' %.10e, on the oracle's %.10e)  trace %.10e  |T| %.3e (spectral radius %.3e)" % (
                dev, sl, lam_dev[lam_dev > 1e-8].sum(), lam[lam > 1e-8].sum(), tr, T, rho))
            gate(0.0 <= dev < 1e-7, name + ": dev")
            gate(abs(tr - np.trace(As)) <= 1e-10 * np.abs(np.diag(As)).sum(), name + ": trace")
            gate(abs(sl - lam_dev[lam_dev > 1e-8].sum()) <= 1e-9 * n * T + 1e-10 * abs(sl) + n * 1e-8, name + ": sum lambda against LAPACK on the device's A'")
            if name not in NOT_GATEABLE:
                tA = gA if len(o["ref"]) == 2 else NUMPY_GATES[0]
                gate(abs(sl - lam[lam > 1e-8].sum()) <= n * tA * np.linalg.norm(o["ref"][0]["A_schur"]) + n * 1e-8, name + ": sum lambda against the oracle's A'")
            gate(rho * (1 - 1e-3) <= T <= 3.0 * rho * (1 + 1e-3), name + ": |T|")
    finally:
        with capfd.disabled():
            print("\n" + "\n".join(notes))
    assert not fails, fails


def _solved_oracles(wins):
    """the C oracle behind its own solve and gauge fix, as tests/test_gpu_bench_shape.py compares the benchmark's launch shape"""
    import bench
    if "solved" not in _CACHE:
        out = []
        for w in wins:
            O = orc.Window(w); so = O.solve(bench.SOLVER_ITERATIONS, True); x = O.states()
            R0 = NO.q2R(np.asarray(w["pose"])[0, 3:]); P0 = np.asarray(w["pose"])[0, :3]
            Rs, Ps, Vs, po = orc.gauge_fix(R0, P0, x["pose"], x["sb"])
            sb = x["sb"].copy(); sb[:, :3] = Vs
            pref, dbg = orc.Window(dict(w, pose=po, speedbias=sb, ex_pose=x["ex"], lam=x["lam"])).marginalize_old()
            out.append(dict(ref=[dbg], lam=_spectrum(dbg["A_schur"]), n=pref["n"], m=pref["m"], trace=(list(so.dogleg_case), list(so.step_ok), so.num_iterations)))
        _CACHE["solved"] = out
    return _CACHE["solved"]


@pytest.mark.parametrize("nt", ["256", "512"])
def test_eigen_solver_chains_behind_the_solve(gpu, monkeypatch, nt):
    """the benchmark windows marginalised behind the device's solve and gauge fix: the clustered spectra of a second-generation prior"""
    wins = bench_windows(gpu)
    names = ["bench%d" % k for k in range(16)]
    orcs = _solved_oracles(wins)
    notes = check_properties("solved", names, orcs, None)
    fails = []
    monkeypatch.setenv("TCV_MARG_NT", nt)
    runs = []
    for order in (None, None, list(range(len(wins)))[::-1]):
        b, pos, hold = marginalise(gpu, wins, order, solve=True)
        assert list(b.marg_status()) == [0] * len(wins)
        runs.append((b, pos, hold))
    monkeypatch.setenv("TCV_MARG_NT", "512")
    b2, pos2, hold2 = marginalise(gpu, wins, solve=True)
    b, pos, hold = runs[0]
    s = b.summaries()
    for k, (name, o) in enumerate(zip(names, orcs)):
        d = b.prior(k).export(); As, bs = b.prior(k).schur()
        d2 = b2.prior(k).export(); As2, bs2 = b2.prior(k).schur()
        JtJ, Jtr = d["J0"].T @ d["J0"], d["J0"].T @ d["r0"]
        JtJ2, Jtr2 = d2["J0"].T @ d2["J0"], d2["J0"].T @ d2["r0"]
        dog, ok, ni = o["trace"]
        same_trace = s[k].num_iterations == ni and [s[k].dogleg_case[i] for i in range(ni)] == dog[:ni] and [s[k].step_ok[i] for i in range(ni)] == ok[:ni]
        r = o["ref"][0]
        notes.append("%s nt %s behind the solve: J0'J0 vs A' %.2e  J0'r0 vs b' %.2e  between shapes J0'J0 %.2e J0'r0 %.2e |b'|  vs the C oracle A' %.2e b' %.2e  same trace %s" % (
            name, nt, fro(JtJ, As), fro(Jtr, bs), fro(JtJ, JtJ2), np.linalg.norm(Jtr - Jtr2) / np.linalg.norm(bs), fro(As, r["A_schur"]), fro(bs, r["b_schur"]), same_trace))
        if not np.array_equal(As, As2) or not np.array_equal(bs, bs2):
            fails.append(name + ": A', b' differ between the shapes")
        if not (fro(JtJ, As) < 2e-6 and fro(Jtr, bs) < 5e-5):
            fails.append(name + ": J0'J0 = A', J0'r0 = b'")
        if not (fro(JtJ, JtJ2) < 1e-9 and np.linalg.norm(Jtr - Jtr2) <= 1e-7 * np.linalg.norm(bs)):
            fails.append(name + ": J0'J0, J0'r0 between the shapes")
        if not ((d["m"], d["n"]) == (o["m"], o["n"]) and same_trace and fro(As, r["A_schur"]) < 4e-6 and fro(bs, r["b_schur"]) < 3e-6):
            fails.append(name + ": the solve's trace, A', b' against the C oracle")
        for other, opos, _ in runs[1:]:
            c = other.prior(opos[k]).export()
            if not (np.array_equal(d["J0"], c["J0"]) and np.array_equal(d["r0"], c["r0"]) and len(d["x0"]) == len(c["x0"]) and all(np.array_equal(x, y) for x, y in zip(d["x0"], c["x0"]))):
                fails.append(name + ": J0, r0, x0 differ between two runs")
    print("\n" + "\n".join(notes))
    assert not fails, fails


@pytest.mark.parametrize("nt", ["256", "512"])
def test_eigen_solver_chains_are_deterministic(gpu, monkeypatch, nt):
    """the same batch twice, and once with the windows in reversed order (other workgroups, other neighbours on the CU, another slice of
    the global scratch): J0, r0, x0 of every window bit for bit.  A race between the two lanes of an eigenvector, or a read of the
    scratch before its store is visible, shows up here."""
    wins = bench_windows(gpu) + cases(gpu, "bench")[1] + cases(gpu, "ragged")[1]
    monkeypatch.setenv("TCV_MARG_NT", nt)
    runs = []
    for order in (None, None, list(range(len(wins)))[::-1]):
        b, pos, hold = marginalise(gpu, wins, order)
        assert list(b.marg_status()) == [0] * len(wins)
        runs.append([b.prior(pos[k]).export() for k in range(len(wins))])
    for other in runs[1:]:
        for k, (a, c) in enumerate(zip(runs[0], other)):
            assert np.array_equal(a["J0"], c["J0"]) and np.array_equal(a["r0"], c["r0"]), k
            assert len(a["x0"]) == len(c["x0"]) and all(np.array_equal(x, y) for x, y in zip(a["x0"], c["x0"])), k
