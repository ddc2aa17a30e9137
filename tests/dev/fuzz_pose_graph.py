#!/usr/bin/env python3
"""Developer checker (GPU): tcv_pose_graphs_optimize on seeded random graph structures against tests/pose_graph_oracle.py.  Per seed: a node
count on and around the band's chunk and panel sizes, 0 .. 20 random loop edges (shared newer ends, loops to constant nodes), one of four
sequence layouts, a start yaw next to the +-180 degree wrap, three drift levels, exact or noisy loop measurements, and grossly wrong
loops that switch the Huber loss on.  Every case is solved alone and again sixteen at a time in ragged batches: the traces must be identical
to the oracle's, the figures inside the gates of tests/test_gpu_pose_graph.py, and solo and batch bit-identical.

A case whose oracle solve comes within 1 % of one of its own thresholds (pose_graph_oracle.decision_margin) is listed and skipped: there the
device may legitimately decide otherwise.  More than 2 % skipped fails the run (tests/test_pose_graph_cpu.py holds the generator to that on
the CPU).

    python tests/dev/fuzz_pose_graph.py [cases] [first seed]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tc-viml_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_oracle as PO      # noqa: E402

NODES = (2, 3, 5, 6, 9, 17, 33, 60, 78, 82, 120)      # free band unknowns 4 (n - 1): below, on and past PG_LD = 20; 308 and 324 past the first panel
MODES = ("one sequence", "constant head", "two sequences", "scattered constants")
MARGIN = 0.01
MAX_SKIPPED = 0.02
BATCH = 16


def make_case(seed):
    """(graph, description) of one seed"""
    rng = np.random.default_rng(700000 + seed)
    n = int(rng.choice(NODES))
    loops = []
    for _ in range(int(rng.integers(0, 21))):
        cur = int(rng.integers(1, n)); old = int(rng.integers(0, cur))
        if (cur, old) not in loops:
            loops.append((cur, old))
    mode = MODES[int(rng.integers(len(MODES)))]
    seq, cut = None, 0
    if mode == "constant head":
        cut = int(rng.integers(1, max(2, n // 3) + 1)) if n > 2 else 1
        seq = [0] * cut + [1] * (n - cut)
    elif mode == "two sequences":
        cut = int(rng.integers(1, n))
        seq = [1] * cut + [2] * (n - cut)
    elif mode == "scattered constants":
        seq = [0 if (i > 0 and rng.random() < 0.15) else 1 for i in range(n)]
    # no sequence edge crosses `cut`: as in the reference, where a sequence joins the graph through a loop, one loop ties the part behind it
    # to the part in front (otherwise that part floats freely and the step along its gauge is rounding noise times the radius)
    if cut and not any(cur >= cut > old for cur, old in loops):
        loops.append((cut, int(rng.integers(0, cut))))
    yaw0 = float(rng.choice([0.0, 150.0, -170.0]))
    drift = float(rng.choice([0.005, 0.02, 0.05]))
    noise = float(rng.choice([0.0, 0.01]))
    bad = tuple(k for k in range(len(loops)) if rng.random() < 0.15)
    g = PO.make_graph(int(rng.integers(1 << 30)), n, loops, sequence=seq, yaw0=yaw0, drift=drift, loop_noise=noise, bad_loops=bad)
    return g, "n %d, %d loops (%d gross), %s, yaw0 %g, drift %g, noise %g" % (n, len(loops), len(bad), mode, yaw0, drift, noise)


def population(cases, seed0):
    """the oracle alone: [(seed, graph, description, oracle result, decision margin)]"""
    out = []
    for seed in range(seed0, seed0 + cases):
        g, what = make_case(seed)
        ref = PO.solve(g)
        out.append((seed, g, what, ref, PO.decision_margin(ref["summary"])))
    return out


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    import tcv_pose_graph as pg
    import test_gpu_pose_graph as T      # compare(), same_bits() and the gates: one definition of "agrees with the oracle"
    pop = population(cases, seed0)
    skipped = [(seed, what, "%.2g of %s at record %d" % m) for seed, _, what, _, m in pop if m[0] < MARGIN]
    live = [c for c in pop if c[4][0] >= MARGIN]
    solo = {seed: pg.optimize([g])[0] for seed, g, _, _, _ in live}
    batch = {}
    for k in range(0, len(live), BATCH):
        part = live[k:k + BATCH]
        batch.update(zip([c[0] for c in part], pg.optimize([c[1] for c in part])))
    tally, worst, bad = {}, {}, []
    for seed, g, what, ref, _ in live:
        term = ref["summary"]["termination"]
        tally[term] = tally.get(term, 0) + 1
        figures = {}
        try:
            T.compare(solo[seed], ref, figures)
            T.compare(batch[seed], ref, figures)
            assert T.same_bits(solo[seed], batch[seed]), "solo and batch differ"
        except AssertionError as e:
            bad.append((seed, what, "trace: " + str(e)[:300]))
            continue
        for k, v in figures.items():
            if v > worst.get(k, (-1.0, 0))[0]:
                worst[k] = (v, seed)
        over = T.exceeded(figures, T.FUZZ_GATES)
        if over:
            bad.append((seed, what, "gate: " + ", ".join("%s %.2e" % kv for kv in over.items())))
    print("by termination:", dict(sorted(tally.items())), " invalid steps:", sum(any(i["step"] < 0 for i in c[3]["summary"]["iterations"]) for c in pop))
    print("worst (seed):", {k: "%.1e (%d)" % v for k, v in worst.items()})
    print("skipped (within %g of a threshold): %d of %d" % (MARGIN, len(skipped), cases))
    for x in skipped:
        print("  ", x)
    print("flagged:", len(bad))
    for x in bad[:20]:
        print("  ", x)
    return 1 if bad or len(skipped) > MAX_SKIPPED * cases else 0


if __name__ == "__main__":
    sys.exit(main())
