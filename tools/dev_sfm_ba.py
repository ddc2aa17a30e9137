#!/usr/bin/env python3
"""Developer tool (GPU): timing of tcv_sfm_ba for batches of problems of the reference's shape (F = 11, 150 points, about 7 observations
each; seeded, tests/sfm_ba_oracle.make_problem), the figures of profiles/sfm_ba.txt.

    python tools/dev_sfm_ba.py [batch sizes ...]      (default 1 64 1024)

Wall = the whole call on the host clock (it ends in the wait for the download); the device parts from events on the call's stream."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tc-viml_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import sfm_ba_oracle as BO      # noqa: E402
import tcv_sfm_ba as ba         # noqa: E402

WARMUP, TIMED = 3, 10


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1, 64, 1024]
    pool = [ba.Problem(BO.make_problem(5000 + k, F=11, n_points=150, l=k % 10, visible=0.55)) for k in range(max(sizes))]
    st = ba.plan_stats(pool[0])
    print("problems of F = 11, 150 points, %.1f observations per point (first problem: %d), %d camera unknowns, LDS %d bytes, scratch %.2f MB per problem"
          % (np.mean([p.count.mean() for p in pool]), st["observations"], st["camera_unknowns"], st["lds_bytes"], st["scratch_bytes"] / 1e6))
    print("%d warm-up calls, %d timed calls; wall = the whole call on the host clock, the device parts from events on the call's stream" % (WARMUP, TIMED))
    print("problems     wall ms median [min, max]   ms / problem      pack   upload    kernel  download   recs mean [min, max]   accepted")
    for n in sizes:
        descs = [p.desc for p in pool[:n]]
        wall, parts = [], []
        for k in range(WARMUP + TIMED):
            t0 = time.perf_counter()
            rc, out, res = ba.bundle_adjust_raw(descs)
            t1 = time.perf_counter()
            assert rc == 0, rc
            if k >= WARMUP:
                wall.append(1e3 * (t1 - t0))
                t = ba.last_timing()
                parts.append([t["pack_ms"], t["upload_ms"], t["kernel_ms"], t["download_ms"]])
        recs = np.array([res[k].summary.iterations for k in range(n)])
        acc = sum(res[k].summary.accepted for k in range(n))
        m = np.median(np.array(parts), 0)
        print("%8d   %9.3f [%8.3f, %8.3f]   %12.4f  %8.3f %8.3f %9.3f %9.3f   %5.1f [%d, %d]   %d of %d"
              % (n, np.median(wall), min(wall), max(wall), np.median(wall) / n, m[0], m[1], m[2], m[3], recs.mean(), recs.min(), recs.max(), acc, n))


if __name__ == "__main__":
    main()
