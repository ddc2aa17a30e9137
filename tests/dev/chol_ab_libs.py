"""Developer A/B (GPU): the solved states and cost traces of two builds of the library, compared bit for bit, on the windows that reach the
edges of the tiled Cholesky and the back substitution (tests/test_gpu_chol_chain.py: 2, 5, 7 frames, four benchmark windows, a
relocalisation window) in every launch shape -- a handful of windows (cooperative instance), the same on one workgroup each (chain
instance), 300 windows (two workgroups per CU) -- plus the golden window in the dense layout at 256 and 512 threads, and one lock-step
frame of replay windows.  Prints the solve kernel's time of one benchmark window and of the replay frame for both builds.

    python tests/dev/chol_ab_libs.py tc-viml_amd/libtcv_hip_prev.so tc-viml_amd/libtcv_hip.so
"""
import os, subprocess, sys, pickle
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) == 3 and sys.argv[1] == "--child":
    for p in ("tc-viml_amd", "tools", "tests", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, p))
    sys.path.insert(0, ROOT)
    import numpy as np
    import synth, tcv, bench
    from relo_util import add_relocalisation, hip_relo_window
    from util import golden_windows, sub_window
    out_file = sys.argv[2]
    sys.argv = sys.argv[:1]      # (dev_small_batch reads its own command line)
    import dev_small_batch as dsb

    def run(wins, wg=0, threads=256, variant=0):
        tcv.lib().tcv_set_solver_variant(variant)
        try:
            made = [hip_relo_window(tcv, w) if "relo" in w else (tcv.Window(w), None) for w in wins]
            b = tcv.Batch([m[0] for m in made])
            b.solve(tcv.default_options(8, True, True, threads, True, wg)); b.synchronize(); b.download_states()
            s = b.summaries()
            return [dict(pose=W.pose.copy(), sb=W.sb.copy(), ex=W.ex.copy(), lam=W.lam.copy(), relo=None if r is None else r.copy(),
                         cost=np.array([s[k].cost[i] for i in range(s[k].num_iterations)]), step=np.array(b.first_step(k)), workgroups=b.cooperative()["last_solve_workgroups"])
                    for k, (W, r) in enumerate(made)]
        finally:
            tcv.lib().tcv_set_solver_variant(0)

    base = synth.window_at(synth.make_windows(400, 1), 0)
    shapes = {"f2": [sub_window(base, 2)], "f5": [sub_window(base, 5)], "f7": [sub_window(base, 7)],
              "bench": bench.build_batches(tcv, synth, 100000, 4)[1],
              "relo": [add_relocalisation(dict(synth.window_at(synth.make_windows(9300, 1, with_lines=False), 0), prior=None), f=6, seed=2)]}
    out = {}
    for name, wins in shapes.items():
        for wg in (0, 1):
            out[name + " small batch, workgroups_per_window %d" % wg] = run(wins, wg)
        out[name + " batch of 300"] = run([wins[k % len(wins)] for k in range(300)])
    pre, main, z = golden_windows()
    for th in (256, 512):
        out["golden, dense layout, %d threads" % th] = run([pre, main], threads=th, variant=1)
    pairs = dsb.replay_windows(dsb.FRAME)
    b, rW, rM = dsb.make_batch(pairs)
    o = tcv.default_options(8, True)
    t = []
    for _ in range(12):
        b.solve(o); b.synchronize(); t.append(b.stats()["solve_ms"])
    b.download_states()
    out["replay frame"] = [dict(pose=W.pose.copy(), sb=W.sb.copy(), lam=W.lam.copy()) for W in rW]
    out["replay_solve_ms"] = float(np.median(t[2:]))
    one = bench.build_batches(tcv, synth, 100000, 1)[0]
    for wg in (0, 1):
        t = []
        ow = tcv.default_options(8, True, True, 256, False, wg)
        for _ in range(14):
            one.solve(ow); one.synchronize(); t.append(one.stats()["solve_ms"])
        out["one_window_solve_ms wg=%d" % wg] = float(np.median(t[2:]))
    pickle.dump(out, open(out_file, "wb"))
    sys.exit(0)
res = []
for k, lib in enumerate(sys.argv[1:3]):
    f = "/tmp/chol_ab_%d.pkl" % k
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", f], env=dict(os.environ, TCV_LIB=os.path.abspath(lib)))
    res.append(pickle.load(open(f, "rb")))
import numpy as np


def same(a, c):
    if isinstance(a, dict):
        return all(same(a[k], c[k]) for k in a)
    if a is None or c is None:
        return a is None and c is None
    return np.array_equal(a, c)


ok = True
for key, val in res[0].items():
    if isinstance(val, list):
        eq = len(val) == len(res[1][key]) and all(same(a, c) for a, c in zip(val, res[1][key]))
        ok = ok and eq
        print("%-50s windows %3d  workgroups %s  bit-identical: %s" % (key, len(val), val[0].get("workgroups", "-"), eq))
    else:
        print("%-50s %.4f -> %.4f ms" % (key, val, res[1][key]))
sys.exit(0 if ok else 3)
