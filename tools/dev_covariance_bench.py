#!/usr/bin/env python3
"""Time of tcv_batch_compute_covariance (tc-viml_amd/csrc/tcv_cov.hip) on the benchmark batch -- the windows bench.py builds -- next to
tcv_batch_evaluate and tcv_batch_solve in the same run, with HIP events on the launch stream.

    python tools/dev_covariance_bench.py [--windows 1024] [--reps 20] [--out profiles/covariance.txt] [--landmarks]

Two request lists: the newest pose (6 solved columns), and every pose of the window (66 solved columns), each at the solved states.
--landmarks adds tcv_batch_compute_landmark_covariance (include/tcv_landmark_covariance.h) with the same camera blocks as cross blocks --
none, the newest pose, every pose -- so that each landmark row stands beside the plain call that solves the same columns.
The result replaces the "== timing" section of the output file (the rest of profiles/covariance.txt is kept).  Needs a HIP device."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tc-viml_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MARK = "== timing"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance.txt"))
    ap.add_argument("--landmarks", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import synth
    import tcv
    import tcv_covariance as cv
    if tcv.lib().tcv_device_count() < 1:
        raise SystemExit("dev_covariance_bench.py needs a HIP device")
    B = args.windows
    batch, wins, keep = bench.build_batches(tcv, synth, bench.shard_ids(0, B), B)
    opts = tcv.default_options(bench.SOLVER_ITERATIONS, True)
    F = batch.windows[0].pose.shape[0]
    newest = [("pose", -1)]
    every = [("pose", i) for i in range(F)]

    def timed(fn):
        ms = []
        for _ in range(3):
            fn()
        batch.synchronize()
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            batch.synchronize(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    rows = [("solve, %d iterations" % bench.SOLVER_ITERATIONS, timed(lambda: batch.solve(opts))),
            ("evaluate at the solution, cost + gradient", timed(lambda: batch.evaluate("solution", gradient=True))),
            ("covariance at the solution, newest pose (6 columns)", timed(lambda: cv.compute(batch, newest, at_solution=True))),
            ("covariance at the solution, every pose (%d columns)" % (6 * F), timed(lambda: cv.compute(batch, every, at_solution=True)))]
    if args.landmarks:
        import tcv_landmark_covariance as lc
        rows += [("landmark covariance at the solution, no cross block", timed(lambda: lc.compute(batch, [], at_solution=True))),
                 ("landmark covariance at the solution, newest pose (6 columns)", timed(lambda: lc.compute(batch, newest, at_solution=True))),
                 ("landmark covariance at the solution, every pose (%d columns)" % (6 * F), timed(lambda: lc.compute(batch, every, at_solution=True)))]
    st = cv.status(batch)
    sig = cv.block_all(batch, F - 1)[:, [0, 1, 2], [0, 1, 2]] ** 0.5
    ps = batch.plan_stats()
    lines = [MARK + ": tcv_batch_compute_covariance on the benchmark batch: %d windows, %d plans, %s on %s" % (B, ps["num_plans"], tcv.lib().tcv_version().decode(), torch.cuda.get_device_name(0)),
             "HIP events on the launch stream around one call, median (min .. max) of %d calls after 3 warm-up calls [ms]" % args.reps]
    for name, (med, lo, hi) in rows:
        lines.append("  %-56s %8.3f  (%.3f .. %.3f)" % (name, med, lo, hi))
    lines += ["windows with status 0: %d of %d; median position sigma of the newest pose: %.3g m" % (int((st == 0).sum()), B, float(statistics.median(sig.mean(1)))),
              "one workgroup per CU (the packed triangle of S fills the LDS), a persistent grid walks the batch; untuned, no phase breakdown measured yet"]
    if args.landmarks:
        lst, var = lc.status(batch), lc.variances_all(batch)
        nl = [lc.n_landmarks(batch, w) for w in range(B)]
        rel = [float(statistics.median(var[w, :nl[w]] ** 0.5 / batch.windows[w].lam[:nl[w]])) for w in range(B) if lst[w] == 0 and nl[w] > 0]
        lines.append("landmark call: windows with status 0: %d of %d; landmarks per window %d .. %d; median sigma(inverse depth) / inverse depth: %.3g"
                     % (int((lst == 0).sum()), B, min(nl), max(nl), float(statistics.median(rel)) if rel else float("nan")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    head = ""
    if os.path.exists(args.out):
        head = open(args.out).read().split(MARK)[0]
    with open(args.out, "w") as f:
        f.write(head + text)


if __name__ == "__main__":
    main()
