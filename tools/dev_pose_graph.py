#!/usr/bin/env python3
"""First numbers of the batched 4-DoF pose-graph optimisation (tcv_pose_graphs_optimize, tc-viml_amd/csrc/tcv_pose_graph.hip).

    python tools/dev_pose_graph.py [--nodes 750] [--loops 100] [--batches 1,8,128] [--reps 10] [--out profiles/pose_graph.txt]

Writes: the parity of every test graph against the NumPy restatement (the figures the gates of tests/test_gpu_pose_graph.py are three
times of), milliseconds per batch and per graph for batches of graphs with --nodes keyframes and --loops loop edges (a 150 s sequence
with every second frame a keyframe), the split between host packing, upload, kernel and download, the scratch bytes per graph, and --
where SciPy is present -- the same graphs through a Levenberg-Marquardt loop on one CPU core whose step is a sparse factorisation
(SuperLU).  Warm-up runs first, then --reps timed runs; median, minimum and maximum are stated.  Needs a HIP device."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tc-viml_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def restatement():
    """tests/pose_graph_oracle.py: the test graphs, their generator and the restated solve (measurement only: the product never sees it)"""
    import pose_graph_oracle
    return pose_graph_oracle


def bench_graph(PO, seed, n, loops):
    import numpy as np
    rng = np.random.default_rng(seed)
    cur = sorted(rng.choice(np.arange(n // 5, n), loops, replace=False))
    return PO.make_graph(seed, n, [(int(c), int(rng.integers(1, c - n // 10))) for c in cur], drift=0.005, loop_noise=0.01)


def parity(PO, pg, out):
    import numpy as np
    out.append("parity against tests/pose_graph_oracle.py, every test graph solved alone (absolute unless stated)")
    out.append("%-26s %5s %4s  %9s %9s %9s %9s %9s %9s" % ("graph", "recs", "term", "cost rel", "rho", "t [m]", "R", "yaw_drift", "t_drift"))
    worst = {}
    for name, g in PO.test_graphs().items():
        d, r = pg.optimize([g])[0], PO.solve(g)
        s, so = d["summary"], r["summary"]
        n = len(so["iterations"])
        same = (s["iterations"], list(s["step"]), s["termination"]) == (n, [i["step"] for i in so["iterations"]], so["termination_code"])
        a = np.array([i["cost"] for i in so["iterations"]] + [i["cost_candidate"] for i in so["iterations"]])
        b = np.concatenate([s["cost"][:n], s["cost_candidate"][:n]])
        f = dict(cost_rel=float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300) * (np.abs(a) > 1e-20))),
                 rho=float(np.max(np.abs(np.array([i["rho"] for i in so["iterations"]]) - s["rho"][:n]))),
                 t=float(np.abs(d["t"] - r["t"]).max()), R=float(np.abs(d["R"] - r["R"]).max()),
                 yaw_drift=abs(s["yaw_drift"] - so["yaw_drift"]), t_drift=float(np.abs(s["t_drift"] - so["t_drift"]).max()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
        out.append("%-26s %5d %4d  %9.2e %9.2e %9.2e %9.2e %9.2e %9.2e%s" % (name, s["iterations"], s["termination"], f["cost_rel"], f["rho"], f["t"], f["R"],
                                                                          f["yaw_drift"], f["t_drift"], "" if same else "   TRACE DIFFERS"))
    out.append("%-26s %5s %4s  %9.2e %9.2e %9.2e %9.2e %9.2e %9.2e" % ("worst", "", "", worst["cost_rel"], worst["rho"], worst["t"], worst["R"], worst["yaw_drift"], worst["t_drift"]))
    out.append("")


def cpu_sparse(PO, g):
    """the restated Levenberg-Marquardt loop with a sparse Jacobian and a sparse direct step; returns (records, seconds in the
    factorisation and solve, seconds in all)"""
    import numpy as np
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    C = PO.CERES_DEFAULTS
    G = PO.Graph(g)
    nf = 4 * len(G.free)

    def linearize(x):
        rows, cols, vals, r, cost = [], [], [], np.zeros(4 * len(G.red)), 0.0
        for n, (k, a, b, m) in enumerate(G.red):
            c, re, Ja, Jb = PO.edge(k, x[a], x[b], m, G.opt)
            cost += c; r[4 * n:4 * n + 4] = re
            for node, J in ((a, Ja), (b, Jb)):
                if not G.const[node]:
                    rr, cc = np.meshgrid(np.arange(4 * n, 4 * n + 4), np.arange(G.col[node], G.col[node] + 4), indexing="ij")
                    rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(J.ravel())
        return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * len(G.red), nf)), r, cost

    t_all = time.perf_counter()
    t_step = 0.0
    x = G.x0()
    J, r, cost = linearize(x)
    scale = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel()))
    radius, dec, recs = C["initial_trust_region_radius"], 2.0, 1
    for _ in range(G.opt["max_num_iterations"]):
        recs += 1
        t0 = time.perf_counter()
        Js = J @ sp.diags(scale)
        diag = np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), C["min_lm_diagonal"], C["max_lm_diagonal"])
        step = -spl.splu((Js.T @ Js + sp.diags(diag / radius)).tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0).solve(Js.T @ r)
        t_step += time.perf_counter() - t0
        Jstep = Js @ step
        mcc = -float(Jstep @ (r + Jstep / 2.0))
        xc = G.plus(x, step * scale)
        cand = G.cost(xc)
        if abs(cost - cand) <= C["function_tolerance"] * cost:
            break
        rho = (cost - cand) / mcc
        if rho > C["min_relative_decrease"]:
            x = xc
            J, r, cost = linearize(x)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)); dec = 2.0
        else:
            radius /= dec; dec *= 2.0
    return recs, t_step, time.perf_counter() - t_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=750)
    ap.add_argument("--loops", type=int, default=100)
    ap.add_argument("--batches", default="1,8,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph.txt"))
    args = ap.parse_args()
    import tcv
    import tcv_pose_graph as pg
    if tcv.lib().tcv_device_count() < 1:
        raise SystemExit("dev_pose_graph.py needs a HIP device")
    PO = restatement()
    out = ["tcv_pose_graphs_optimize: first numbers (tools/dev_pose_graph.py)", ""]
    parity(PO, pg, out)
    sizes = [int(v) for v in args.batches.split(",")]
    graphs = [bench_graph(PO, 1000 + k, args.nodes, args.loops) for k in range(max(sizes))]
    G = [pg.Graph(g) for g in graphs]
    st = pg.plan_stats(G[0])
    out.append("timing: graphs of %d nodes, %d loop edges: %d free nodes, band %d, border %d, %d edges, scratch %.2f MB per graph" % (
        args.nodes, args.loops, st["free"], st["band"], st["border"], st["edges"], st["scratch_bytes"] / 1e6))
    out.append("3 warm-up calls, %d timed calls; wall = the whole call on the host clock, the device parts from events on the call's stream" % args.reps)
    out.append("%7s  %28s  %10s  %8s %8s %9s %9s  %5s" % ("graphs", "wall ms median [min, max]", "ms / graph", "pack", "upload", "kernel", "download", "recs"))
    for B in sizes:
        descs = [g.desc for g in G[:B]]
        wall, parts = [], []
        for rep in range(3 + args.reps):
            t0 = time.perf_counter()
            rc, _, _, sums = pg.optimize_raw(descs)
            t1 = time.perf_counter()
            tcv.check(rc)
            if rep >= 3:
                wall.append(1e3 * (t1 - t0)); parts.append(pg.last_timing())
        med = statistics.median(wall)
        pm = {k: statistics.median(p[k] for p in parts) for k in parts[0]}
        out.append("%7d  %10.3f [%8.3f, %8.3f]  %10.3f  %8.3f %8.3f %9.3f %9.3f  %5.1f" % (B, med, min(wall), max(wall), med / B, pm["pack_ms"], pm["upload_ms"],
                                                                                           pm["kernel_ms"], pm["download_ms"], sum(s.iterations for s in sums[:B]) / B))
    out.append("")
    try:
        import scipy  # noqa: F401
        ts = [cpu_sparse(PO, g) for g in graphs[:3]]
        out.append("one CPU core, the restated loop with a sparse Jacobian and SuperLU for the step (scipy %s), 3 graphs:" % scipy.__version__)
        out.append("  factorisation + solve: %.2f ms per graph (%.2f ms per LM iteration); whole loop incl. the edge maths in Python: %.0f ms per graph" % (
            1e3 * statistics.mean(t[1] for t in ts), 1e3 * sum(t[1] for t in ts) / sum(t[0] - 1 for t in ts), 1e3 * statistics.mean(t[2] for t in ts)))
    except ImportError:
        out.append("SciPy is not installed here: no CPU figure")
    text = "\n".join(out) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
