#!/usr/bin/env python3
"""Developer checker (GPU): tcv_sfm_ba on seeded random problem structures against tests/sfm_ba_oracle.py.  Per seed: a frame count from 2
to TCV_SFM_BA_MAX_FRAMES, any reference frame (l = F - 1 included), a point count on and around the Schur chunk of 16, a visibility from
"two frames each" to "nearly all", sometimes a frame no point sees, and three noise levels.  Every case is solved alone and again all
together in one ragged batch: the traces must be identical to the oracle's, the figures inside the gates of tests/test_gpu_sfm_ba.py, and
solo and batch bit-identical.  Every case must decide at least MARGIN clear of each of its thresholds (sfm_ba_oracle.decision_margin):
tests/test_gpu_sfm_ba.py runs seeds 0 .. 29, which do.

    python tests/dev/fuzz_sfm_ba.py [cases] [first seed]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tc-viml_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import sfm_ba_oracle as BO      # noqa: E402

FRAMES = (2, 3, 4, 5, 7, 11, 15)
POINTS = (1, 2, 7, 15, 16, 17, 33, 48, 70)
MARGIN = 1e-6


def make_case(seed):
    """(problem, description) of one seed"""
    rng = np.random.default_rng(900000 + seed)
    F = int(rng.choice(FRAMES))
    l = int(rng.integers(0, F))
    n = int(rng.choice(POINTS))
    visible = float(rng.choice([0.0, 0.3, 0.7, 0.95]))
    blind = ()
    if F >= 4 and rng.random() < 0.25:
        blind = (int(rng.choice([f for f in range(F) if f != l])),)
    pose_noise, point_noise = [(0.01, 0.03), (0.02, 0.05), (0.06, 0.2)][int(rng.integers(3))]
    p = BO.make_problem(int(rng.integers(1 << 30)), F=F, n_points=n, l=l, pose_noise=pose_noise, point_noise=point_noise, visible=visible, blind_frames=blind)
    return p, "F %d, l %d, %d points, visible %g, blind %s, noise %g / %g" % (F, l, n, visible, blind, pose_noise, point_noise)


def population(cases, seed0):
    """the oracle alone: [(seed, problem, description, oracle result, decision margin)]"""
    out = []
    for seed in range(seed0, seed0 + cases):
        p, what = make_case(seed)
        ref = BO.solve(p)
        out.append((seed, p, what, ref, BO.decision_margin(ref["summary"])))
    return out


def run(ba, compare, same_bits, cases, seed0, quiet=False):
    """solo and one ragged batch against the oracle; returns (worst figures, terminations seen)"""
    pop = population(cases, seed0)
    for seed, _, what, _, m in pop:
        assert m[0] >= MARGIN, (seed, what, m)
    solo = {seed: ba.bundle_adjust([p])[0] for seed, p, _, _, _ in pop}
    batch = dict(zip([c[0] for c in pop], ba.bundle_adjust([c[1] for c in pop])))
    worst, tally = {}, {}
    for seed, p, what, ref, m in pop:
        f = {}
        compare(solo[seed], ref, f, p)
        compare(batch[seed], ref, f, p)
        assert same_bits(solo[seed], batch[seed]), (seed, what)
        s = ref["summary"]
        tally[s["termination"]] = tally.get(s["termination"], 0) + 1
        if not quiet:
            print("seed %3d  %-66s records %2d %-22s margin %.1e  " % (seed, what, len(s["iterations"]), s["termination"], m[0]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst, tally


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    import tcv_sfm_ba as ba
    import test_gpu_sfm_ba as T      # compare(), same_bits() and the gates: one definition of "agrees with the oracle"
    worst, tally = run(ba, T.compare, T.same_bits, cases, seed0)
    print("terminations:", tally)
    print("worst:", {k: "%.3g" % v for k, v in worst.items()})
    bad = T.exceeded(worst, T.FUZZ_GATES)
    print("FAIL" if bad else "PASS", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
