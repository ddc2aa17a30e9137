"""Developer A/B (GPU): the marginalisation results of two builds of the library, compared bit for bit, each build in a fresh child process.

    python tests/dev/marg_ab_libs.py tc-viml_amd/libtcv_hip_prev.so tc-viml_amd/libtcv_hip.so [--ms-only]

What runs: the priors of one lock-step frame of replay windows (block mode, chunked projection path) and of the benchmark windows, as
before, and every path of the kernel's body: the cases of tests/marg_plan_cases.py that pack, a rank-deficient dropped block (built as in
tests/test_gpu_marg.py::test_rank_deficient_dropped_block_takes_the_eigen_path) and two dropped sets with 24 < m <= 64 (Cholesky and
forward substitution in LDS), each at the window's own state under TCV_MARG_NT = 256 and 512, plain and under TCV_MARG_PROJ_SERIAL, TCV_MARG_EIG_MM=1 and
TCV_MARG_EIG_FLAGS = 1, 2, 3, and (plain) behind the device's solve.  Compared per run: J0, r0, x0, A', b', the status word,
the count of leading zero rows of J0 | r0 (the second status word is that count; the C-ABI hands it to device consumers only, so it is
taken from J0 here), and the diagnostic slots the TCV_DEBUG dump prints (Jacobi sweeps, trace(Amm^-1), the eigen-solver's self-check).
--ms-only: the child only times the replay frame's marginalisation (for alternating speed runs)."""
import os, pickle, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NTS = ("256", "512")
SWITCHES = ({}, {"TCV_MARG_PROJ_SERIAL": "1"}, {"TCV_MARG_EIG_MM": "1"}, {"TCV_MARG_EIG_FLAGS": "1"}, {"TCV_MARG_EIG_FLAGS": "2"}, {"TCV_MARG_EIG_FLAGS": "3"})
ENV_KEYS = ("TCV_MARG_NT", "TCV_MARG_PROJ_SERIAL", "TCV_MARG_BLOCK_SERIAL", "TCV_MARG_OWN_IMU", "TCV_MARG_OWN_PRIOR", "TCV_MARG_EIG_MM", "TCV_MARG_EIG_FLAGS", "TCV_DEBUG")


def body_cases(tcv, synth, mpc, np):
    """name -> (builder of (solve window, marginalisation problem, drops), packer switches, may run behind a solve)"""
    out = {k: (b, env, True) for k, (b, env) in mpc.cases(tcv).items() if not k.startswith("err_")}

    def rank_deficient():
        w = synth.window_at(synth.make_windows(905, 1, frame_shift=-1), 0)
        pr = w["proj"]
        fi, fj, lm = np.asarray(pr["frame_i"]), np.asarray(pr["frame_j"]), np.asarray(pr["landmark"])
        l0 = int(lm[(fi == 0) & (fj == 1)][0])
        keep = ~((lm == l0) & ~((fi == 0) & (fj == 1)))
        w = dict(w, proj={k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (len(fi),) else v) for k, v in pr.items()})
        pose = np.array(w["pose"], copy=True); pose[1] = pose[0]
        return mpc._old(tcv, dict(w, pose=pose))

    def landmarks(n):      # landmark k is anchored in frame k % 7: m = 6 + 9 + ceil(n / 7), one piece up to m = 64
        return lambda: mpc._old(tcv, synth.window_at(synth.make_windows(906, 1, n_landmarks=n, frame_shift=-1), 0))

    def prior_from_hbm():      # MARGIN_SECOND_NEW with a prior without zero rows: 75 x 75 stored entries do not fit region P (70 x 71), marg_prior reads J0 from HBM
        from util import golden_windows
        main = golden_windows()[1]
        J0 = np.array(main["prior"]["J0"], copy=True)
        zero = np.flatnonzero(~J0.any(axis=1))
        J0[zero, zero] = 1.0
        return mpc._second_new(tcv, dict(main, prior=dict(main["prior"], J0=J0)))

    out["prior_from_hbm"] = (prior_from_hbm, {}, True)
    out["rank_deficient"] = (rank_deficient, {}, False)      # (a solve would move the pose that takes the parallax away)
    out["lds_cholesky_m25"] = (landmarks(70), {}, True)
    out["lds_cholesky_m64"] = (landmarks(343), {}, True)
    return out


def set_env(env):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)


def prior_record(tcv, np, b):
    """everything comparable of window 0's result: arrays, status, derived zero-row count, the diagnostic lines of the TCV_DEBUG dump"""
    rec = {"status": int(b.marg_status()[0])}
    os.environ["TCV_DEBUG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            P = b.prior(0)
        finally:
            os.dup2(saved, 2); os.close(saved); os.environ.pop("TCV_DEBUG", None)
        tf.seek(0)
        dump = tf.read().decode(errors="replace")
    rec["diag"] = [s for s in dump.splitlines() if re.search(r"jacobi sweeps|trace\(Amm|tridiag check", s)]
    d = P.export()
    rec.update(m=d["m"], n=d["n"], J0=d["J0"], r0=d["r0"], x0=np.concatenate([np.atleast_1d(x) for x in d["x0"]]) if d["x0"] else np.zeros(0))
    if d["n"] > 0:
        rec["As"], rec["bs"] = P.schur()
        nz = np.flatnonzero(np.any(d["J0"] != 0, axis=1) | (d["r0"] != 0))
        rec["zero_rows"] = min(int(nz[0]) if len(nz) else d["n"], d["n"] - 1)
    return rec


def child(out_file, ms_only):
    sys.path.insert(0, os.path.join(ROOT, "tc-viml_amd")); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
    import numpy as np
    import synth, tcv, bench
    sys.argv = sys.argv[:1]      # (dev_small_batch reads its own command line)
    import dev_small_batch as dsb
    out = {}
    pairs = dsb.replay_windows(dsb.FRAME)
    b = dsb.make_batch(pairs)[0]
    b.solve(tcv.default_options(8, True)); b.gauge_fix(); b.marginalize(); b.synchronize(); b.download_priors(compact=True)
    out["replay"] = [p.export() for p in b.priors()]
    t = []
    for _ in range(10):
        b.marginalize(); b.synchronize(); t.append(b.stats()["marg_ms"])
    out["replay_marg_ms"] = float(np.median(t))
    if not ms_only:
        batch, wins, keep = bench.build_batches(tcv, synth, 100000, 16)
        batch.solve(tcv.default_options(8, True)); batch.gauge_fix(); batch.marginalize(); batch.synchronize(); batch.download_priors(compact=True)
        out["bench"] = [p.export() for p in batch.priors()]
        import marg_plan_cases as mpc
        body = {}
        for name, (build, pack_env, may_solve) in body_cases(tcv, synth, mpc, np).items():
            for nt in NTS:
                for sw in SWITCHES:
                    for solve in ((False, True) if may_solve and not sw else (False,)):      # (behind the solve: the plain kernel only)
                        key = (name, nt, tuple(sorted(sw.items())), solve)
                        set_env(dict(pack_env, TCV_MARG_NT=nt, **sw))
                        try:
                            W, M, drops = build()
                            bb = tcv.Batch([W], [M], [drops])
                            if solve:
                                bb.solve(tcv.default_options(8, True)); bb.gauge_fix()
                            bb.marginalize(); bb.synchronize()
                            body[key] = prior_record(tcv, np, bb)
                        except tcv.TcvError as e:
                            body[key] = {"error": str(e)}
                        finally:
                            set_env({})
        out["body"] = body
    pickle.dump(out, open(out_file, "wb"))


def same(a, c):
    import numpy as np
    if a.keys() != c.keys():
        return False
    return all(np.array_equal(a[k], c[k]) if isinstance(a[k], np.ndarray) else a[k] == c[k] for k in a)


def main():
    ms_only = "--ms-only" in sys.argv
    libs = [a for a in sys.argv[1:] if not a.startswith("--")]
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, lib in enumerate(libs[:2]):
            f = os.path.join(tmp, "marg_ab_%d.pkl" % k)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", f] + (["--ms-only"] if ms_only else []), env=dict(os.environ, TCV_LIB=os.path.abspath(lib)))
            res.append(pickle.load(open(f, "rb")))
    import numpy as np
    if not ms_only:
        for key in ("replay", "bench"):
            eq = all(np.array_equal(a["J0"], c["J0"]) and np.array_equal(a["r0"], c["r0"]) and all(np.array_equal(x, y) for x, y in zip(a["x0"], c["x0"]))
                     for a, c in zip(res[0][key], res[1][key]))
            print(key, "windows:", len(res[0][key]), "priors bit-identical:", eq)
        A, B = res[0]["body"], res[1]["body"]
        bad = [k for k in A if not same(A[k], B.get(k, {}))]
        names = sorted({k[0] for k in A})
        for name in names:
            runs = [k for k in A if k[0] == name]
            ran = [k for k in runs if "error" not in A[k]]
            refused = sorted({A[k]["error"] for k in runs if "error" in A[k]})
            r0 = A[ran[0]]
            print("  %-22s %3d runs%s  m %d n %d status %s zero rows %s  %s" % (
                name, len(ran), " (+ %d refused: %s)" % (len(runs) - len(ran), "; ".join(refused)) if refused else "", r0["m"], r0["n"],
                sorted({A[k]["status"] for k in ran}), sorted({A[k].get("zero_rows", -1) for k in ran}), "; ".join(s.strip() for s in r0["diag"][:2])))
        for k in bad:
            print("  DIFFERENT:", k, {f for f in A[k] if f not in B.get(k, {}) or not same({f: A[k][f]}, {f: B[k][f]})})
        print("body: %d runs of %d cases (%d refused on both sides alike):" % (len(A), len(names), sum("error" in A[k] for k in A)), "ALL EQUAL" if not bad and A.keys() == B.keys() else "%d DIFFERENT" % len(bad))
    print("marginalisation of the replay frame [ms]:", res[0]["replay_marg_ms"], "->", res[1]["replay_marg_ms"])


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        child(sys.argv[2], "--ms-only" in sys.argv)
    else:
        main()
