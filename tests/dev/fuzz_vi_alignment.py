#!/usr/bin/env python3
"""Developer checker (GPU): the visual-inertial alignment (include/tcv_vi_alignment.h) on seeded random sequences (tests/vi_alignment_cases.py,
fuzz_case: F 4 .. 40, uniform or ragged periods 5 .. 25, dt uniform or per sample, key frames all / sparse / one / random, IMU noise on or
off, scale 0.05 .. 50, gyroscope bias up to 0.1 rad/s, the SfM frame random or within {0, 1e-7, 1e-3, 0.1} rad of +-z, one of two noise
vectors) against the NumPy restatement (tests/vi_alignment_oracle.py) on the device's own pre-integrations.  Every case runs alone and sixteen
at a time in ragged batches whose bits must be the solo bits; the status must be the restatement's, and for an aligned case every output
family must hold e(device) <= 8 u, u = max(e(float64, natural-order Cholesky), e(float64, numpy.linalg.solve), FLOOR), each against long double.

A case is left out (counted, printed) only where the restatement alone is undecided (`undecided`): float64 and long double disagree on the
status, | |g| - G | is within 1 % of 1, |s| is under 100 x its float64-to-long-double difference, or a relative pivot is within MARGIN = 30 of
the gate.  At most 5 % may be left out.  On the CPU (synth / np_oracle pre-integrations, tests/test_vi_alignment_cpu.py) seeds 0 .. 299 leave
out 0 of 300, and so do they on the device.  The default and the suite run seeds 0 .. 59 (worst e(device) / u 6.2).  In the long range (300 from
seed 0) ONE case is over the gate and returns 1, seed 147: scale, Ps, Rs at 8.3, 9.2, 13.5 u with e(device) 1e-14 .. 2e-14 at a condition number of
2.8e7.  The restatement's own float64 error there moves between 2e-16 and 1e-14 under one-ulp changes of T, so both solves behind u sit low; on
Rs that spread (4.6e-15 at most over 20 draws) still leaves a factor of about 2 to the device that is NOT explained.  The gate stays as it is
(profiles/vi_alignment_paths.txt).

    python tests/dev/fuzz_vi_alignment.py [cases] [first seed]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tc-viml_amd")); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import vi_alignment_cases as VC      # noqa: E402
import vi_alignment_oracle as VO      # noqa: E402

LD = np.longdouble
GATE, MARGIN, G = 4e-11, 30.0, 9.81007      # the device's default gate, the project's margin (tests/test_vi_alignment_cpu.py)
FLOOR = 4 * 2.0 ** -53                      # tests/test_gpu_vi_alignment.py
FAMILIES = ("delta_bg", "velocity", "gravity_c0", "gravity", "scale", "Ps", "Rs", "Vs")
BITS = ("status", "delta_bg", "bg", "scale", "gravity_c0", "gravity", "rot_diff", "min_pivot", "velocity", "Ps", "Rs", "Vs")
MAX_LEFT_OUT = 0.05                         # fuzz_solve's cap


def e(x, ref):
    d = float(np.abs(np.asarray(x).astype(LD) - ref).max())
    m = float(np.abs(ref).max())
    return d if m == 0.0 else d / m


def undecided(r64, rld):
    """why the restatement alone does not decide this case (None: it does)"""
    if r64["status"] != rld["status"]:
        return "status float64 %d, long double %d" % (r64["status"], rld["status"])
    for r in (r64, rld):
        piv = [float(p) for p in r["bias_pivots"]] + [float(p) for _, v in r["stages"] for p in v]
        failed = piv.pop() if r["status"] == VO.RANK else None
        if piv and min(piv) < MARGIN * GATE:
            return "a passing pivot %.3g within %g of the gate" % (min(piv), MARGIN)
        if failed is not None and abs(failed) > GATE / MARGIN:
            return "the failing pivot %.3g within %g of the gate" % (failed, MARGIN)
    if r64["bias_status"] != VO.OK or r64["status"] in (VO.RANK, VO.NON_FINITE):
        return None
    lin64, linld = (r64, rld) if r64["status"] == VO.LINEAR else (r64["linear"], rld["linear"])
    for r in (lin64, linld):
        g = np.asarray(r["gravity_c0"])
        if abs(abs(float(np.sqrt(g @ g)) - G) - 1.0) < 0.01:
            return "| |g| - G | within 1 % of 1"
    pairs = [(lin64["scale"], linld["scale"])] + ([(r64["scale"], rld["scale"])] if r64["status"] in (VO.OK, VO.REFINED_SCALE) else [])
    for s64, sld in pairs:
        if abs(float(s64)) < 100.0 * abs(float(LD(s64) - sld)):
            return "s %.3g under 100 x its float64-to-long-double difference" % float(s64)
    return None


def reference(case, preintegrate=VC.preint_np, pre0=None, pre1=None, with_dense=True):
    """(float64, long double, float64 through numpy.linalg.solve or None) restatements at the default gate"""
    kw = dict(preintegrate=preintegrate, gate=GATE, pre0=pre0, pre1=pre1)
    r64, p1 = VC.run_oracle_imu(case, dtype=np.float64, **kw)
    rld, _ = VC.run_oracle_imu(case, dtype=LD, **dict(kw, pre1=pre1 if pre1 is not None else p1))
    rdn = None
    if with_dense and r64["status"] == rld["status"] == VO.OK:
        rdn, _ = VC.run_oracle_imu(case, dtype=np.float64, solver="dense", **dict(kw, pre1=pre1 if pre1 is not None else p1))
    return r64, rld, rdn


def same_bits(a, b):
    bad = [k for k in BITS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    return bad + ["preint." + k for k in a["preint"] if not np.array_equal(a["preint"][k], b["preint"][k])]


def main():
    import tcv
    import tcv_vi_alignment as va
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60      # the suite's range; the long range is 300 from seed 0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    C = [VC.fuzz_case(seed0 + k) for k in range(cases)]
    S = [va.Sequence(c) for c in C]
    solo = [va.align([s], want_preint=True)[0] for s in S]
    bad, left_out, statuses = [], [], {}
    # sixteen at a time, in an order of its own
    order = np.random.default_rng(seed0).permutation(cases)
    for k in range(0, cases, 16):
        idx = order[k:k + 16]
        for i, r in zip(idx, va.align([S[i] for i in idx], want_preint=True)):
            d = same_bits(r, solo[i])
            if d:
                bad.append((C[i]["name"], "batch bits differ", d))
    worst = {f: 0.0 for f in FAMILIES}
    for c, r in zip(C, solo):
        pre0 = VC.preint_tcv(tcv, c["imu"], c["ba0"], c["bg0"], c["noise"])
        r64, rld, rdn = reference(c, pre0=pre0, pre1=r["preint"])
        why = undecided(r64, rld)
        if why:
            left_out.append((c["name"], why))
            print("left out  %s: %s" % (c["name"], why), flush=True)
            continue
        statuses[r64["status"]] = statuses.get(r64["status"], 0) + 1
        if r["status"] != r64["status"]:
            bad.append((c["name"], "status", r["status"], r64["status"]))
            continue
        if r64["status"] != VO.OK:
            zero = [k for k in ("gravity", "rot_diff", "Ps", "Rs", "Vs") if np.asarray(r[k]).any()]
            if zero:
                bad.append((c["name"], "not zero behind status %d" % r["status"], zero))
            continue
        for f in FAMILIES:
            u = max(e(r64[f], rld[f]), e(rdn[f], rld[f]), FLOOR)
            ed = e(r[f], rld[f])
            worst[f] = max(worst[f], ed / u)
            if not ed <= 8 * u:
                bad.append((c["name"], f, "e(device) %.2e" % ed, "u %.2e" % u))
    print("statuses (restatement):", dict(sorted(statuses.items())))
    print("worst e(device) / u per family (gate 8):", {k: "%.2f" % v for k, v in worst.items()})
    print("left out: %d of %d" % (len(left_out), cases))
    if len(left_out) > MAX_LEFT_OUT * cases:
        bad.append(("more than 5 % of the cases left out", len(left_out)))
    print("flagged:", len(bad))
    for x in bad[:20]:
        print("  ", x)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
