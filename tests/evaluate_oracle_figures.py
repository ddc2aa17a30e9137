#!/usr/bin/env python3
"""Not a test: the CPU side of profiles/evaluate_parity.txt: how far the two oracles are from EACH OTHER on the windows of tests/test_gpu_evaluate.py
(np_oracle.Problem.linearize against orc.Window.linearize_dense: cost and gradient J'r), and the directional-derivative figure of the
NumPy oracle's own gradient and cost -- the numbers the device's gaps are read against.  No device needed.

    python tests/evaluate_oracle_figures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tc-viml_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import np_oracle as NO          # noqa: E402
import orc                      # noqa: E402
from evaluate_cases import cases, directional_error, oracle_evaluate          # noqa: E402
from util import fro, rel       # noqa: E402


def main():
    orc.build()
    cs = cases()
    wc = wg = 0.0
    for name, (w, kw) in cs.items():
        if any(w.get(k) is not None for k in ("td", "relo")) or w["line"].get("exact_jacobian"):
            continue          # the C oracle has no ProjectionTdFactor, relocalisation pose or exact line Jacobian
        exc = not kw.get("estimate_extrinsic", True)
        o = oracle_evaluate(w, ex_constant=exc)
        H, g, cost, n, nc = orc.Window(w, ex_constant=exc).linearize_dense()
        dc, dg = rel(o["cost"], cost), max(rel(o["gradient"], g), fro(o["gradient"], g))
        print("%-24s cost %.3e   gradient %.3e" % (name, dc, dg))
        wc, wg = max(wc, dc), max(wg, dg)
    print("NumPy oracle against C oracle, worst: cost %.3e, gradient %.3e" % (wc, wg))
    for name in ("synth_points_only", "line_exact"):
        w, kw = cs[name]
        P = NO.Problem(w)
        x0 = P.x0()
        J, r, c = P.linearize(x0)
        g = J.T @ r
        worst = 0.0
        for seed in range(4):
            d = np.random.default_rng(1000 + seed).normal(size=P.nlocal)
            d /= np.linalg.norm(d)
            worst = max(worst, directional_error(lambda x: P.linearize(x, want_jac=False)[2], g, P.plus, x0, d))
        print("directional derivative, NumPy oracle alone, %-20s worst of 4 seeds %.3e" % (name, worst))


if __name__ == "__main__":
    main()
