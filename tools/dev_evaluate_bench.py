#!/usr/bin/env python3
"""Time of tcv_batch_evaluate (tc-viml_amd/csrc/tcv_eval.hip) on the benchmark batch -- the windows bench.py builds -- next to
tcv_batch_solve in the same run, with HIP events on the launch stream.

    python tools/dev_evaluate_bench.py [--windows 1024] [--reps 20] [--out profiles/evaluate_bench.txt]

Three cases: cost only, cost + gradient, everything (residuals, block costs, gradient), each at the initial states.  The figure to put
beside them is one trust-region iteration of the solve kernel: solve time / iterations of the summary.  Needs a HIP device."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tc-viml_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.txt"))
    args = ap.parse_args()
    import torch
    import bench
    import synth
    import tcv
    if tcv.lib().tcv_device_count() < 1:
        raise SystemExit("dev_evaluate_bench.py needs a HIP device")
    B = args.windows
    batch, wins, keep = bench.build_batches(tcv, synth, bench.shard_ids(0, B), B)
    opts = tcv.default_options(bench.SOLVER_ITERATIONS, True)

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

    rows = [("evaluate, cost only", timed(lambda: batch.evaluate())),
            ("evaluate, cost + gradient", timed(lambda: batch.evaluate(gradient=True))),
            ("evaluate, residuals + block costs + gradient", timed(lambda: batch.evaluate(residuals=True, gradient=True, block_costs=True))),
            ("solve, %d iterations" % bench.SOLVER_ITERATIONS, timed(lambda: batch.solve(opts)))]
    rows.append(("evaluate at the solution, everything", timed(lambda: batch.evaluate("solution", residuals=True, gradient=True, block_costs=True))))
    iters = statistics.mean(s.num_iterations for s in batch.summaries())
    cost = batch.evaluation_costs()[0]
    L = tcv.lib()
    L.tcv_evaluate_kernel_shape.argtypes = [C.c_size_t, C.POINTER(C.c_int)]
    ps = batch.plan_stats()
    lds = 8 * (max(w.pose.size + w.sb.size + w.ex.size + w.lam.size for w in batch.windows) + 1 + 512 + 8 * 450)
    shape = (C.c_int * 4)()
    tcv.check(0 if L.tcv_evaluate_kernel_shape(lds, shape) == 0 else tcv.TCV_ERR_HIP)
    solve_ms = rows[3][1][0]
    lines = ["tcv_batch_evaluate on the benchmark batch: %d windows, %d plans, %s on %s" % (B, ps["num_plans"], L.tcv_version().decode(), torch.cuda.get_device_name(0)),
             "HIP events on the launch stream around one call, median (min .. max) of %d calls after 3 warm-up calls [ms]" % args.reps]
    for name, (med, lo, hi) in rows:
        lines.append("  %-48s %8.3f  (%.3f .. %.3f)" % (name, med, lo, hi))
    lines += ["one trust-region iteration of the solve kernel in this run: %.3f ms / %.2f iterations = %.3f ms per %d windows" % (solve_ms, iters, solve_ms / iters, B),
              "launch shape of evaluate_kernel: grid %d x 256 threads, about %d bytes of dynamic LDS, %d VGPRs, %d bytes of scratch per thread;" % (B, lds, shape[0], shape[2]),
              "  resident workgroups per CU reported by the runtime: %d (%d waves per SIMD); solve kernel: grid %d, %d bytes of LDS" % (shape[3], shape[3], ps["grid"], ps["lds_bytes"]),
              "mean cost of the batch at the solution: %.6g" % float(cost.mean())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
