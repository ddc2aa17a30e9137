"""Developer tool (GPU): the chain elimination of the solve kernel step by step -- per interval between two step barriers, how long each
of the four wavefronts takes from the previous barrier to its arrival at this one, and how often it is the last to arrive.  Needs one
profile build per wavefront (csrc/tcv_solve.hip, TCV_PROFILE_CHAIN):

    for w in 0 1 2 3; do python tc-viml_amd/build.py --suffix=cs$w -DTCV_PROFILE=1 -DTCV_PROFILE_CHAIN=$w; done
    python tools/dev_chain_steps.py cs

Shapes: the benchmark window (11 frames, device-made prior, 12 intervals; 1024 windows, two workgroups per CU) and the 2-, 5- and 7-frame
windows of tests/test_gpu_chol_chain.py (300 copies each).  Cycles are means per chain; `last` is the share of the chains in which the
wavefront arrived last.  Wavefronts 0, 1: column owners; 2: matrix cores; 3: T pipeline."""
import os, pickle, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["bench", "f2", "f5", "f7"]
if len(sys.argv) == 3 and sys.argv[1] == "--child":
    for p in ("tc-viml_amd", "tests", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, p))
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import synth, tcv, bench
    from util import sub_window
    L = tcv.lib(); L.tcv_batch_profile.argtypes = [C.c_void_p, tcv._dp]
    base = synth.window_at(synth.make_windows(400, 1), 0)
    res = {}
    for name in SHAPES:
        if name == "bench":
            b = bench.build_batches(tcv, synth, 100000, 1024)[0]
        else:
            w = sub_window(base, int(name[1:]))
            keep = [tcv.Window(w) for _ in range(300)]
            b = tcv.Batch(keep)
        o = tcv.default_options(8, True)
        out = np.zeros(32)
        b.solve(o); b.synchronize(); L.tcv_batch_profile(b.h, tcv.dptr(out))      # (warm-up, cleared)
        b.solve(o); b.synchronize(); L.tcv_batch_profile(b.h, tcv.dptr(out))
        res[name] = (out.copy(), b.stats()["solve_ms"])
    pickle.dump(res, open(sys.argv[2], "wb"))
    sys.exit(0)
tabs = []
for w in range(4):
    f = "/tmp/chain_steps_%d.pkl" % w
    lib = os.path.join(ROOT, "tc-viml_amd", "libtcv_hip_%s%d.so" % (sys.argv[1], w))
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", f], env=dict(os.environ, TCV_LIB=lib))
    tabs.append(pickle.load(open(f, "rb")))
for name in SHAPES:
    chains = [tabs[w][name][0][26] for w in range(4)]
    n = max(s for s in range(13) if tabs[0][name][0][s] > 0) + 1
    print("%s: %d intervals, %.0f chains, solve kernel %.3f ms (profile build)" % (name, n, chains[0], tabs[0][name][1]))
    print("  interval |   cycles to arrival: w0     w1     w2     w3 |  slowest | arrived last: w0    w1    w2    w3")
    tot = [0.0] * 4; slow = 0.0
    for s in range(n):
        cyc = [tabs[w][name][0][s] / chains[w] for w in range(4)]
        last = [tabs[w][name][0][13 + s] / chains[w] for w in range(4)]
        tot = [a + c for a, c in zip(tot, cyc)]; slow += max(cyc)
        print("  %8d | %25.0f %6.0f %6.0f %6.0f | %8.0f | %16.2f %5.2f %5.2f %5.2f" % ((s,) + tuple(cyc) + (max(cyc),) + tuple(last)))
    print("  %8s | %25.0f %6.0f %6.0f %6.0f | %8.0f |" % (("sum",) + tuple(tot) + (slow,)))
