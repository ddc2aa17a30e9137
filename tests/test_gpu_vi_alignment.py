"""The visual-inertial alignment on the device (include/tcv_vi_alignment.h) against the NumPy restatement (tests/vi_alignment_oracle.py) in
float64 and long double, on the inputs of tests/vi_alignment_cases.py.

Parity inputs: the call's optional `preint` output must be bit-identical to tcv_preintegrate on the same samples at (0, bg); the restatement
then runs on those pre-integrations, and its gyroscope bias on tcv_preintegrate's at (ba0, bg0), so that only the new code is compared.

Parity gate, per output family: with e(x) = max |x - x_longdouble| / max |x_longdouble|, e(device) <= max(8 e(float64 restatement), FLOOR) --
the factor tests/test_gpu_landmark_covariance.py uses."""
import numpy as np
import pytest

import vi_alignment_cases as VC
import vi_alignment_oracle as VO

pytestmark = pytest.mark.gpu
LD = np.longdouble
# The floor, for families whose float64 error is zero (gravity after the rotation is (0, 0, G); Ps of a single key frame is exactly 0): the
# long-double reference rounded to the device's float64 is itself off by up to 2^-53 of the family's largest entry (half an ulp of 1..2),
# and a float64 result that is exact up to its last operation (a 3 x 3 rotation: two additions on three products) by three more.
FLOOR = 4 * 2.0 ** -53
FAMILIES = ("delta_bg", "velocity", "gravity_c0", "gravity", "scale", "Ps", "Rs", "Vs")
BITS = ("status", "delta_bg", "bg", "scale", "gravity_c0", "gravity", "rot_diff", "min_pivot", "velocity", "Ps", "Rs", "Vs")
# sizes built into the kernel (tc-viml_amd/csrc/tcv_align.h): AL_THREADS = 64 lanes -- 3 F = 63 | 66 unknowns at F = 21 | 22, 63 | 64 | 65 intervals at
# F = 64 | 65 | 66, 63 | 64 | 65 frames and key frames; TCV_VI_ALIGN_MAX_FRAMES = 128 at F = 127 | 128
assert set(VC.GPU_FRAMES) >= {4, 5, 11, 21, 22, 64, 65, 128} | {63, 66, 127}


@pytest.fixture(scope="module")
def va(gpu):
    import tcv_vi_alignment
    return tcv_vi_alignment


@pytest.fixture(scope="module")
def cases():
    return VC.gpu_cases()


@pytest.fixture(scope="module")
def solo(va, cases):
    """every case aligned alone, with the re-propagated pre-integrations: computed once, shared, never changed"""
    return [va.align([c], want_preint=True)[0] for c in cases]


def _same_bits(a, b, what):
    for k in BITS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)
    if "preint" in a and "preint" in b:
        for k in a["preint"]:
            assert np.array_equal(a["preint"][k], b["preint"][k]), (what, "preint", k)


def _e(x, ref):
    d = float(np.abs(np.asarray(x).astype(LD) - ref).max())
    m = float(np.abs(ref).max())
    return d if m == 0.0 else d / m      # (Ps of a single key frame is exactly zero on every side)


def test_shapes_cover_periods_subsets_and_a_single_key_frame(cases):
    assert [len(c["R"]) for c in cases][:len(VC.GPU_FRAMES)] == list(VC.GPU_FRAMES)
    assert {c["period"] for c in cases} == {10, 20}
    nk = [(len(c["key_frame"]), len(c["R"])) for c in cases]
    assert any(k == 1 for k, _ in nk) and any(k == F for k, F in nk) and any(1 < k < F for k, F in nk)


def test_preint_output_is_tcv_preintegrate_at_zero_ba_and_bg(gpu, cases, solo):
    for c, r in zip(cases, solo):
        assert r["status"] == VO.OK, c["name"]
        assert np.array_equal(r["bg"], c["bg0"] + r["delta_bg"])
        acc, gyr, dt = VC.imu_arrays(c)
        n = len(acc)
        ref = gpu.preintegrate(acc, gyr, dt, np.zeros((n, 3)), np.tile(r["bg"], (n, 1)), VC.NOISE)
        for k in ref:
            assert np.array_equal(ref[k], r["preint"][k]), (c["name"], k)
        assert not r["preint"]["lin_ba"].any() and np.array_equal(r["preint"]["lin_bg"], np.tile(r["bg"], (n, 1)))


def test_parity_per_family_against_long_double(gpu, cases, solo):
    worst = {}
    failures = []
    for c, r in zip(cases, solo):
        acc, gyr, dt = VC.imu_arrays(c)
        n = len(acc)
        pre0 = gpu.preintegrate(acc, gyr, dt, np.tile(c["ba0"], (n, 1)), np.tile(c["bg0"], (n, 1)), VC.NOISE)
        r64 = VO.align(c["R"], c["T"], c["tic"], r["preint"], c["key_frame"], dtype=np.float64)
        rld = VO.align(c["R"], c["T"], c["tic"], r["preint"], c["key_frame"], dtype=LD)
        r64["delta_bg"] = VO.gyro_bias(c["R"], pre0, np.float64)[0]
        rld["delta_bg"] = VO.gyro_bias(c["R"], pre0, LD)[0]
        assert r64["status"] == rld["status"] == VO.OK, c["name"]
        line = []
        for f in FAMILIES:
            ed, e64 = _e(r[f], rld[f]), _e(r64[f], rld[f])
            line.append("%s %.1e/%.1e" % (f, ed, e64))
            worst[f] = max(worst.get(f, 0.0), ed / max(8 * e64, FLOOR))
            if not ed <= max(8 * e64, FLOOR):
                failures.append((c["name"], f, ed, e64))
        print("%-26s device/float64: %s" % (c["name"], "  ".join(line)))
        # the smallest relative pivot the device met is the restatement's, to the gate's precision (a ratio, far from the gate: 30 x)
        assert 0.5 <= r["min_pivot"] / float(min(r64["pivots"].min(), 1.0)) <= 2.0, (c["name"], r["min_pivot"], float(r64["pivots"].min()))
    print("worst e(device) / max(8 e(float64), floor) per family:", {k: "%.2f" % v for k, v in worst.items()})
    assert not failures, failures


def test_status_codes(va, cases, solo):
    for F in (2, 3):
        for S in (10, 20):
            r = va.align([VC.make_case(3 + F, F, S)], want_preint=True)[0]
            assert r["status"] == va.RANK, (F, S, r["status"])
            # the bias and the pre-integrations are there, everything behind them is zero
            assert r["delta_bg"].any() and r["preint"]["delta_p"].any()
            assert not any(np.asarray(r[k]).any() for k in ("scale", "gravity_c0", "gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"))
    c = dict(cases[2])      # F = 11
    neg = dict(c, T=-c["T"])
    r = va.align([neg])[0]
    assert r["status"] == va.LINEAR and r["scale"] < 0 and abs(np.linalg.norm(r["gravity_c0"]) - 9.81007) < 1.0      # s < 0 (:184)
    assert not any(np.asarray(r[k]).any() for k in ("gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"))
    assert abs(r["scale"] + solo[2]["scale"]) < 1e-3 * solo[2]["scale"]
    r = va.align([c], va.default_options(gravity_norm=5.0))[0]
    assert r["status"] == va.LINEAR and r["scale"] > 0 and abs(np.linalg.norm(r["gravity_c0"]) - 5.0) > 1.0      # | |g| - G | > 1 (:184)
    assert not any(np.asarray(r[k]).any() for k in ("gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"))


def test_a_failing_sequence_leaves_its_neighbours_bits(va, cases, solo):
    idx = [0, 3, 7, None, 2, 10, 5]
    batch = [VC.make_case(6, 3, 20) if i is None else cases[i] for i in idx]
    res = va.align(batch, want_preint=True)
    assert [r["status"] for r in res] == [0, 0, 0, va.RANK, 0, 0, 0]
    for i, r in zip(idx, res):
        if i is not None:
            _same_bits(r, solo[i], cases[i]["name"])


def test_bits_do_not_depend_on_the_batch(va, cases, solo):
    assert len(cases) == 13
    fwd = va.align(cases, want_preint=True)
    rev = va.align(cases[::-1], want_preint=True)[::-1]
    for c, s, a, b in zip(cases, solo, fwd, rev):
        _same_bits(a, s, c["name"] + " in the batch")
        _same_bits(b, s, c["name"] + " in the reversed batch")
    again = va.align([cases[4]], want_preint=True)[0]
    _same_bits(again, solo[4], "run to run")


def test_timing_is_reported(va, cases):
    va.align(cases[:3])
    t = va.last_timing()
    assert all(v >= 0 for v in t.values()) and t["align_kernel_ms"] > 0 and t["bias_kernel_ms"] > 0 and t["align_ms"] >= t["align_kernel_ms"]
