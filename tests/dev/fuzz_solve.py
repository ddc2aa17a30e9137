#!/usr/bin/env python3
"""Developer checker (GPU): randomised window STRUCTURES through the fused solve against the C oracle (oracle/ is the checker here, as in
tests/).  Every case is a seeded mutation of a golden or synthetic window -- ragged tracks, landmarks seen once, few or no points / lines,
short windows, IMU factors left out (sum_dt > 10 s), constant extrinsics, with and without the prior -- solved four ways on the device:

    lone      a batch of one (cooperative kernels when the window is large enough for helpers, 160 KiB of LDS)
    single    a batch of one with TCV_COOP_H=0 (one workgroup, 160 KiB)
    packed    257 copies (a batch larger than the chip: two workgroups per CU, 80 KiB each)
    dense     tcv_set_solver_variant(1): the dense layout

and compared with the oracle: first step (no trust-region decision behind it) to 1e-6, then trace, final cost and states.  A window whose
trust-region decisions are borderline may legitimately take another branch; such cases are listed as `trace` and their first step still
has to agree.  Mutations produce ill-posed windows too (a pose seen by one feature and no IMU factor, landmarks seen once at no parallax, two
frames without a prior): there the answer is set by rounding in directions only the trust region's mu D^2 holds.  The checker measures
that on the ORACLE ALONE -- the same window with its states moved by 1e-13 relative, three draws -- and allows the device 30x the oracle's
own movement where that exceeds 1e-6 (`ok~`: listed with the measured sensitivity).  First step and states are held to that rule as a
whole AND within every parameter family (positions, rotations, velocities, accelerometer and gyro biases, extrinsic translation and
rotation, inverse depths), each family relative to the oracle's own magnitude in it and priced by the oracle's own movement in it.

A `trace` verdict is not free: it is excused only when the ORACLE'S OWN trace (iterations, termination, dogleg cases, accepts) changes in at
least one of twelve draws of that 1e-13 noise (`oracle_trace_moves`, drawn lazily) -- otherwise it counts as a mismatch --, and at most
TRACE_CAP = 5 % of the cases of any setting may be `trace` at all (a cap, not a measurement: the oracle's own trace moved in 1 of 120 windows
under three draws, the device's recorded share is at most 2 %, profiles/r05_fuzz_solve.txt, r06_fuzz_solve.txt).

With `convergence` as the third argument every solve -- device and oracle -- runs (50, to convergence) with the Ceres tolerances instead of
(8, fixed); the sensitivity solves are then run lazily, only for a case that exceeds a gate.

    python tests/dev/fuzz_solve.py [cases] [first seed] [convergence]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tc-viml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import np_oracle as NO      # noqa: E402
import orc      # noqa: E402
import synth    # noqa: E402
import tcv      # noqa: E402
from util import fro, fro_by_family, golden_windows, rel, rel_by_family, state_families, sub_window, tangent_families      # noqa: E402

TOL = 1e-6
TRACE_CAP = 0.05            # the share of `trace` verdicts any setting may have
TRACE_DRAWS = 12            # draws of 1e-13 noise in which the oracle's own trace has to move for a `trace` verdict to be excused


def take(d, keep, n):
    return {k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and np.asarray(v).shape[:1] == (n,) else v) for k, v in d.items()}


def thin_points(rng, w, mode):
    pr = {k: np.asarray(v) if isinstance(v, (list, np.ndarray)) else v for k, v in w["proj"].items()}
    n = len(pr["landmark"])
    if n == 0:
        return w
    keep = np.ones(n, bool)
    lm = pr["landmark"]
    for l in np.unique(lm):
        idx = np.nonzero(lm == l)[0]
        if mode == "prefix":
            keep[idx[int(rng.integers(1, len(idx) + 1)):]] = False
        elif mode == "once":
            keep[idx[1:]] = False
        elif mode == "random":
            k = rng.random(len(idx)) < 0.5
            if not k.any():
                k[int(rng.integers(len(idx)))] = True
            keep[idx] = k
        elif mode == "few":      # most landmarks vanish altogether
            if rng.random() < 0.8:
                keep[idx] = False
    out = dict(w)
    out["proj"] = take(pr, keep, n)
    used = sorted(set(int(l) for l in out["proj"]["landmark"]))
    remap = {l: i for i, l in enumerate(used)}
    out["proj"]["landmark"] = np.array([remap[int(l)] for l in out["proj"]["landmark"]], int)
    out["lam"] = np.asarray(w["lam"])[used] if used else np.zeros(0)
    return out


def thin_lines(rng, w, frac):
    ln = w["line"]
    n = len(ln["frame"])
    keep = rng.random(n) < frac
    out = dict(w)
    out["line"] = take(ln, keep, n)
    return out


def make_case(rng, seed):
    pre, main, z = golden_windows()
    # (seeds from 100000 on also draw `chained`: a synthetic window on the prior the ORACLE makes from the window one frame earlier -- priors of
    # many layouts next to every mutation; the list below 100000 is unchanged so that the recorded seed ranges keep their cases)
    kind = rng.choice(["main", "pre", "synth", "synth", "short"] + (["chained", "chained", "chained"] if seed >= 100000 else []))
    notes = [str(kind)]
    if kind == "main":
        w = dict(main)
    elif kind == "pre":
        w = dict(pre)
    elif kind == "chained":
        nl = int(rng.choice([3, 17, 50, 120, 200])); nn = int(rng.choice([1, 7, 40, 100]))
        before = dict(synth.window_at(synth.make_windows(40000 + seed, 1, n_landmarks=nl, n_lines=nn, frame_shift=-1), 0), prior=None)
        Op = orc.Window(before); Op.solve(8, True); st = Op.states()
        before = dict(before, pose=st["pose"], speedbias=st["sb"], ex_pose=st["ex"], lam=st["lam"])
        po, _ = orc.Window(before).marginalize_old()
        w = dict(synth.window_at(synth.make_windows(40000 + seed, 1, n_landmarks=nl, n_lines=nn), 0), prior=po)
        notes.append(f"L{nl} n{nn} prior n={po['n']}")
    else:
        nl = int(rng.choice([1, 3, 17, 50, 120, 200, 290]))
        nn = int(rng.choice([0, 1, 7, 40, 100]))
        w = dict(synth.window_at(synth.make_windows(40000 + seed, 1, n_landmarks=nl, n_lines=max(nn, 1)), 0), prior=None)
        if nn == 0:
            w = thin_lines(rng, w, 0.0)
        notes.append(f"L{nl} n{nn}")
        if kind == "short":
            f = int(rng.integers(2, 11))
            w = sub_window(w, f)
            notes.append(f"frames {f}")
    mode = str(rng.choice(["full", "prefix", "once", "random", "few"]))
    if mode != "full":
        w = thin_points(rng, w, mode)
    notes.append(mode)
    if rng.random() < 0.4:
        fr = float(rng.choice([0.0, 0.1, 0.5]))
        w = thin_lines(rng, w, fr)
        notes.append(f"lines x{fr}")
    gone = []
    nimu = len(w["imu"]["sum_dt"])
    if nimu > 1 and rng.random() < 0.35:
        gone = sorted(set(int(g) for g in rng.integers(0, nimu, size=int(rng.integers(1, 3)))))
        notes.append(f"imu gone {gone}")
    exc = bool(rng.random() < 0.25)
    if exc:
        notes.append("ex const")
    w_hip, w_orc = w, w
    if gone:
        im = dict(w["imu"])
        sd = np.array(im["sum_dt"], dtype=float).copy(); sd[gone] = 11.0; im["sum_dt"] = sd
        w_hip = dict(w, imu=im)
        keep = ~np.isin(np.arange(nimu), gone)
        w_orc = dict(w, imu=take(w["imu"], keep, nimu))
    return w_hip, w_orc, exc, " ".join(notes)


def perturbed(w_orc, rep):
    """the window with its states moved by 1e-13 relative, draw `rep`"""
    r2 = np.random.Generator(np.random.PCG64(977 + rep))
    w2 = dict(w_orc)
    for key in ("lam", "pose", "speedbias"):
        a = np.asarray(w_orc[key], dtype=float)
        w2[key] = a * (1 + 1e-13 * r2.standard_normal(a.shape))
    return w2


def trace_of(s):
    n = min(s.num_iterations, len(s.step_ok))
    return (s.num_iterations, s.termination, [s.dogleg_case[i] for i in range(1, n)], [s.step_ok[i] for i in range(1, n)])


def oracle_trace_moves(w_orc, exc, so0, iters=8, fixed=True, draws=TRACE_DRAWS):
    """does the oracle's own trace change under 1e-13 state noise?  Stops at the first draw in which it does."""
    t0 = trace_of(so0)
    for rep in range(draws):
        if trace_of(orc.Window(perturbed(w_orc, rep), ex_constant=exc).solve(iters, fixed)) != t0:
            return True
    return False


class LazySensitivity:
    """oracle_sensitivity when first asked for (convergence mode: three more oracle solves to convergence per case, needed only where a
    gate is exceeded); `tangent`, which every comparison reads, does not need them"""

    def __init__(self, w_orc, exc, so0, st0, iters, fixed):
        self.args, self.d = (w_orc, exc, so0, st0, iters, fixed), None
        self.tangent = tangent_families(NO.Problem(w_orc, ex_constant=exc))

    def __getitem__(self, key):
        if key == "tangent":
            return self.tangent
        if self.d is None:
            self.d = oracle_sensitivity(*self.args)
        return self.d[key]


def oracle_sensitivity(w_orc, exc, so0, st0, iters=8, fixed=True):
    """how far the oracle's own first step / final cost / states move when the window's states move by 1e-13 relative; `first_family` and
    `state_family`: the same within every parameter family (util.tangent_families / util.state_families); `tangent`: the index sets"""
    f0 = np.array(so0.first_delta[:so0.n_local])
    sens = dict(first=0.0, cost=0.0, pose=0.0, sb=0.0, ex=0.0, lam=0.0, first_family={}, state_family={},
                tangent=tangent_families(NO.Problem(w_orc, ex_constant=exc)))

    def worst(into, d):
        for name, v in d.items():
            into[name] = max(into.get(name, 0.0), v)
    for rep in range(3):
        O = orc.Window(perturbed(w_orc, rep), ex_constant=exc); so = O.solve(iters, fixed)
        f1 = np.array(so.first_delta[:so.n_local])
        if len(f0):
            sens["first"] = max(sens["first"], fro(f1, f0))
            worst(sens["first_family"], fro_by_family(f1, f0, sens["tangent"]))
        sens["cost"] = max(sens["cost"], abs(so.final_cost - so0.final_cost) / max(so0.final_cost, 1e-12))
        st = O.states()
        for key in ("pose", "sb", "ex", "lam"):
            sens[key] = max(sens[key], rel(st[key], st0[key]))
        worst(sens["state_family"], rel_by_family(state_families(st), state_families(st0)))
    return sens


def compare(W, b, s, k, O, so, sens):
    """('ok' | 'ok~' | 'trace' | 'FIRST STEP' | 'STATE', detail)"""
    fo = np.array(so.first_delta[:so.n_local]); fg = b.first_step(k)
    if len(fg) != len(fo):
        return "FIRST STEP", f"length {len(fg)} vs {len(fo)}"
    soft = []
    d1 = fro(fg, fo) if len(fo) else 0.0
    if not d1 < TOL:
        if not d1 < 30 * sens["first"]:
            return "FIRST STEP", f"first step differs {d1:.2e} (oracle moves {sens['first']:.1e})"
        soft.append(f"first step {d1:.1e} / oracle {sens['first']:.1e}")
    for name, d in (fro_by_family(fg, fo, sens["tangent"]) if len(fo) else {}).items():
        if not d < TOL:
            m = sens["first_family"].get(name, 0.0)
            if not d < 30 * m:
                return "FIRST STEP", f"first step differs in {name} {d:.2e} (oracle moves {m:.1e})"
            soft.append(f"first step {name} {d:.1e} / oracle {m:.1e}")
    n = min(so.num_iterations, len(s.step_ok))
    same = s.num_iterations == so.num_iterations and s.termination == so.termination and \
        [s.dogleg_case[i] for i in range(1, n)] == [so.dogleg_case[i] for i in range(1, n)] and [s.step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
    if not same:
        return "trace", f"iterations {s.num_iterations} vs {so.num_iterations}"
    dc = abs(s.final_cost - so.final_cost) / max(so.final_cost, 1e-12)      # (a zero-residual window: absolute below 1e-12)
    if not dc <= TOL:
        if not dc < 30 * sens["cost"]:
            return "STATE", f"final cost {s.final_cost:.9e} vs {so.final_cost:.9e} (oracle moves {sens['cost']:.1e})"
        soft.append(f"cost {dc:.1e} / oracle {sens['cost']:.1e}")
    st, sg = O.states(), W.states()
    for key in ("pose", "sb", "ex", "lam"):
        r = rel(sg[key], st[key])
        if not r < TOL:
            if not r < 30 * sens[key]:
                return "STATE", f"{key} differs {r:.2e} (oracle moves {sens[key]:.1e})"
            soft.append(f"{key} {r:.1e} / oracle {sens[key]:.1e}")
    for name, r in rel_by_family(state_families(sg), state_families(st)).items():
        if not r < TOL:
            m = sens["state_family"].get(name, 0.0)
            if not r < 30 * m:
                return "STATE", f"{name} differs {r:.2e} (oracle moves {m:.1e})"
            soft.append(f"{name} {r:.1e} / oracle {m:.1e}")
    return ("ok~", "; ".join(soft)) if soft else ("ok", "")


def gpu_run(w, exc, copies, coop_off=False, dense=False, mfma=True, iters=8, fixed=True, threads=256, workgroups_per_window=0):
    L = tcv.lib()
    old = os.environ.get("TCV_COOP_H")
    if coop_off:
        os.environ["TCV_COOP_H"] = "0"
    if dense:
        L.tcv_set_solver_variant(1)
    try:
        Ws = [tcv.Window(w, estimate_extrinsic=not exc) for _ in range(copies)]
        b = tcv.Batch(Ws)
        b.solve(tcv.default_options(iters, fixed, mfma, threads, True, workgroups_per_window))
        b.synchronize(); b.download_states()
        return Ws, b, b.summaries()
    finally:
        if dense:
            L.tcv_set_solver_variant(0)
        if coop_off:
            if old is None:
                os.environ.pop("TCV_COOP_H", None)
            else:
                os.environ["TCV_COOP_H"] = old


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    convergence = len(sys.argv) > 3 and sys.argv[3] == "convergence"
    iters, fixed = (50, False) if convergence else (8, True)
    tally = {}
    bad = []
    kept = []
    moves = {}

    def judge(seed, note, name, verdict, detail, w_orc, exc, so):
        """counts a verdict; a `trace` the oracle's own trace does not excuse is a mismatch"""
        if verdict == "trace":
            if seed not in moves:
                moves[seed] = oracle_trace_moves(w_orc, exc, so, iters, fixed)
            if not moves[seed]:
                verdict, detail = "TRACE", detail + f": the oracle's own trace holds in {TRACE_DRAWS} draws of 1e-13 noise"
        tally[(name, verdict)] = tally.get((name, verdict), 0) + 1
        if verdict in ("FIRST STEP", "STATE", "ERROR", "TRACE"):
            bad.append((seed, note, name, verdict, detail))
        return verdict, detail
    for c in range(cases):
        seed = seed0 + c
        rng = np.random.Generator(np.random.PCG64(seed))
        w_hip, w_orc, exc, note = make_case(rng, seed)
        try:
            O = orc.Window(w_orc, ex_constant=exc)
            so = O.solve(iters, fixed)
            sens = LazySensitivity(w_orc, exc, so, O.states(), iters, fixed) if convergence else oracle_sensitivity(w_orc, exc, so, O.states())
        except Exception as e:      # noqa: BLE001
            print(f"case {seed} [{note}]: oracle refused: {e}")
            continue
        kept.append((seed, note, w_hip, exc, O, so, sens, w_orc))
        row = []
        for name, kw in (("lone", dict(copies=1)), ("single", dict(copies=1, coop_off=True)), ("packed", dict(copies=257)), ("dense", dict(copies=1, dense=True))):
            try:
                Ws, b, s = gpu_run(w_hip, exc, iters=iters, fixed=fixed, **kw)
                k = len(Ws) - 1
                verdict, detail = compare(Ws[k], b, s[k], k, O, so, sens)
                lay = b.plan_stats()["layout"]
            except Exception as e:      # noqa: BLE001
                verdict, detail, lay = "ERROR", str(e)[:120], "?"
            verdict, detail = judge(seed, note, name, verdict, detail, w_orc, exc, so)
            row.append(f"{name}:{verdict}" + (f"({detail})" if detail else "") + f"[{lay}]")
        np_, nl_, nlm = len(w_hip["proj"]["landmark"]), len(w_hip["line"]["frame"]), len(w_hip["lam"])
        print(f"case {seed} [{note}; {np_} point, {nl_} line factors, {nlm} landmarks, prior {'yes' if w_hip.get('prior') is not None else 'no'}]: " + "  ".join(row), flush=True)
    # the same windows six at a time in ONE batch (a lock-step frame: different structures side by side, the helpers sized by the largest
    # window, groups rotated over the XCDs), each against its own oracle solve
    for g0 in range(0, len(kept), 6):
        grp = kept[g0:g0 + 6]
        try:
            Ws = [tcv.Window(w, estimate_extrinsic=not exc) for (_, _, w, exc, _, _, _, _) in grp]
            b = tcv.Batch(Ws)
            b.solve(tcv.default_options(iters, fixed, True, 256, True)); b.synchronize(); b.download_states()
            ss = b.summaries()
            for k, (seed, note, w, exc, O, so, sens, w_orc) in enumerate(grp):
                verdict, detail = compare(Ws[k], b, ss[k], k, O, so, sens)
                judge(seed, note, "mixed", verdict, detail, w_orc, exc, so)
            print(f"mixed batch of seeds {[g[0] for g in grp]}: layout {b.plan_stats()['layout']}, plans {b.plan_stats()['num_plans']}, cooperative {b.cooperative()}", flush=True)
        except Exception as e:      # noqa: BLE001
            tally[("mixed", "ERROR")] = tally.get(("mixed", "ERROR"), 0) + 1
            bad.append((grp[0][0], "batch", "mixed", "ERROR", str(e)[:160]))
    for name in sorted(set(a for (a, _) in tally)):      # the cap on `trace` verdicts, excused or not, per setting
        total = sum(n for (a, _), n in tally.items() if a == name)
        traces = tally.get((name, "trace"), 0) + tally.get((name, "TRACE"), 0)
        if traces > TRACE_CAP * total:
            bad.append((seed0, "all cases", name, "TRACE CAP", f"{traces} of {total} cases took another trace than the oracle (cap {TRACE_CAP:.0%})"))
    print("\nmode:", f"({iters}, {'fixed' if fixed else 'to convergence'})")
    print("tally:", {f"{a}/{b}": n for (a, b), n in sorted(tally.items())})
    print("mismatches:", len(bad))
    for x in bad:
        print("  ", x)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
