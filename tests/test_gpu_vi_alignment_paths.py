"""The visual-inertial alignment on the device (include/tcv_vi_alignment.h) off its well-posed path: the exact branches of TangentBasis and
g2R, every status with its zero pattern, and the host's grouping of the pre-integration passes -- on the inputs that
tests/test_vi_alignment_cpu.py has shown decisive on the restatement alone (tests/vi_alignment_cases.py, tests/vi_alignment_oracle.py).

Conventions of tests/test_gpu_vi_alignment.py: the restatement runs on the call's own `preint` output, its gyroscope bias on tcv_preintegrate
at (ba0, bg0); parity per output family, e(device) <= max(8 e(float64 restatement), FLOOR) against long double.  Host paths are compared
bit for bit with the same sequences aligned alone (whose bits the parity tests gate)."""
import ctypes as C

import numpy as np
import pytest

import vi_alignment_cases as VC
import vi_alignment_oracle as VO
from vi_alignment_cases import DEFAULT_GATE, RANK_SITES, SINGULAR_FRAMES, STATUS2, TILTED, VERTICAL

pytestmark = pytest.mark.gpu
LD = np.longdouble
FLOOR = 4 * 2.0 ** -53      # tests/test_gpu_vi_alignment.py
FAMILIES = ("delta_bg", "velocity", "gravity_c0", "gravity", "scale", "Ps", "Rs", "Vs")
BITS = ("status", "delta_bg", "bg", "scale", "gravity_c0", "gravity", "rot_diff", "min_pivot", "velocity", "Ps", "Rs", "Vs")
G = 9.81007
# what a status leaves zero (the header's table); `preint` and the bias are zero only where the bias solve itself failed
BEHIND = {VO.LINEAR: ("gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"), VO.REFINED_SCALE: ("gravity", "rot_diff", "Ps", "Rs", "Vs"),
          VO.RANK: ("scale", "gravity_c0", "gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs"),
          VO.NON_FINITE: ("scale", "gravity_c0", "gravity", "rot_diff", "velocity", "Ps", "Rs", "Vs")}
COMPUTED = {VO.LINEAR: ("delta_bg", "scale", "gravity_c0"), VO.REFINED_SCALE: ("delta_bg", "scale", "gravity_c0", "velocity"), VO.RANK: ("delta_bg",),
            VO.NON_FINITE: ("delta_bg",)}


@pytest.fixture(scope="module")
def va(gpu):
    import tcv_vi_alignment
    return tcv_vi_alignment


def _same_bits(a, b, what):
    for k in BITS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)
    if "preint" in a and "preint" in b:
        for k in a["preint"]:
            # (equal_nan: behind a huge accelerometer the covariance of a pre-integration overflows -- NaN is a value of tcv_preintegrate's there)
            assert np.array_equal(a["preint"][k], b["preint"][k], equal_nan=True), (what, "preint", k)


def _e(x, ref):
    d = float(np.abs(np.asarray(x).astype(LD) - ref).max())
    m = float(np.abs(ref).max())
    return d if m == 0.0 else d / m


def _no_period(c):
    return {k: v for k, v in c.items() if k not in ("period", "acc", "gyr")}


def _reference(gpu, c, r, gate=DEFAULT_GATE):
    """the float64 and long-double restatements on the device's own pre-integrations"""
    pre0 = VC.preint_tcv(gpu, c["imu"], c["ba0"], c["bg0"], c["noise"])
    return [VC.run_oracle_imu(c, dtype=dt, gate=gate, pre0=pre0, pre1=r["preint"])[0] for dt in (np.float64, LD)]


def _parity(c, r, r64, rld, families, worst=None):
    line, failures = [], []
    for f in families:
        ed, e64 = _e(r[f], rld[f]), _e(r64[f], rld[f])
        line.append("%s %.1e/%.1e" % (f, ed, e64))
        if worst is not None:
            worst[f] = max(worst.get(f, 0.0), ed / max(8 * e64, FLOOR))
        if not ed <= max(8 * e64, FLOOR):
            failures.append((c["name"], f, ed, e64))
    print("%-26s device/float64: %s" % (c["name"], "  ".join(line)))
    assert not failures, failures


def _preint_is_tcv_preintegrate(gpu, c, r):
    ref = VC.preint_tcv(gpu, c["imu"], np.zeros(3), r["bg"], c["noise"])
    for k in ref:
        assert np.array_equal(ref[k], r["preint"][k], equal_nan=True), (c["name"], "preint", k)


def _align_each(va, S, want, options=None):
    """va.align over Sequence objects with `preint` asked for per sequence; only what _same_bits reads is unpacked"""
    n = len(S)
    arr = (va.Desc * n)(*[s.desc for s in S])
    res = (va.Result * n)()
    outs = [va.Outputs(s.F, len(s.key), w) for s, w in zip(S, want)]
    for k, o in enumerate(outs):
        o.bind(res[k])
    va.check(va.lib().tcv_vi_align(n, arr, C.byref(options) if options is not None else None, res, None))
    out = []
    for s, r, o, w in zip(S, res, outs, want):
        d = dict(status=int(r.status), delta_bg=np.array(r.delta_bg[:]), bg=np.array(r.bg[:]), scale=float(r.scale), gravity_c0=np.array(r.gravity_c0[:]),
                 gravity=np.array(r.gravity[:]), rot_diff=np.array(r.rot_diff[:]).reshape(3, 3), min_pivot=float(r.min_pivot), velocity=o.velocity, Ps=o.Ps, Rs=o.Rs, Vs=o.Vs)
        if w:
            d["preint"] = va.preint_dict(o.preint, s.F - 1)
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------------------------- exact branches
@pytest.mark.parametrize("F,S,sign", VERTICAL)
def test_vertical_gravity_takes_the_special_tangent_basis_and_both_ends_of_g2R(gpu, va, F, S, sign):
    c = VC.vertical_case(F, S, sign)
    r = va.align([c], want_preint=True)[0]
    assert r["status"] == VO.OK, (c["name"], r["status"])
    # the proof that the branch ran: only a tangent basis of exact unit vectors along x and y keeps the x / y rows decoupled with a zero right-hand
    # side (which of the two is lx does not matter: either order spans the same plane)
    assert r["gravity_c0"][0] == 0 and r["gravity_c0"][1] == 0 and r["gravity_c0"][2] == sign * G, r["gravity_c0"]
    assert not r["delta_bg"].any()
    _preint_is_tcv_preintegrate(gpu, c, r)
    r64, rld = _reference(gpu, c, r)
    assert r64["status"] == rld["status"] == VO.OK and r64["flags"]["tangent_special"] == 4 and bool(r64["flags"].get("g2R_antiparallel")) == (sign < 0)
    _parity(c, r, r64, rld, FAMILIES)
    assert 0.5 <= r["min_pivot"] / r64["min_pivot"] <= 2.0
    if sign < 0:      # the rotation by pi about x, composed with the yaw correction
        assert _e(r["rot_diff"], rld["rot_diff"]) <= max(8 * _e(r64["rot_diff"], rld["rot_diff"]), FLOOR)
        assert np.abs(r["rot_diff"] @ r["gravity_c0"] - [0.0, 0.0, G]).max() <= FLOOR * G


@pytest.mark.parametrize("F,S,delta", TILTED)
def test_gravity_next_to_minus_z_on_both_sides_of_the_antiparallel_threshold(gpu, va, F, S, delta):
    c = VC.tilted_case(F, S, delta)
    r = va.align([c], want_preint=True)[0]
    r64, rld = _reference(gpu, c, r)
    assert r["status"] == r64["status"] == rld["status"] == VO.OK
    assert bool(r64["flags"].get("g2R_antiparallel")) == bool(rld["flags"].get("g2R_antiparallel")) == (delta < 1e-6)
    _parity(c, r, r64, rld, FAMILIES)
    assert _e(r["rot_diff"], rld["rot_diff"]) <= max(8 * _e(r64["rot_diff"], rld["rot_diff"]), FLOOR)


# ---------------------------------------------------------------------------------------------------------------- every status
def _status_inputs():
    """(case, gate, status, site of a rank failure)"""
    out = [(VC.noise_T_case(seed, F), DEFAULT_GATE, VO.REFINED_SCALE, None) for seed, F in STATUS2]
    out += [(_no_period(VC.make_case(7 + F, F, S)), gate, VO.RANK, site) for F, S, gate, site in RANK_SITES]
    for F in SINGULAR_FRAMES[::2]:
        out += [(VC.stationary_case(F), DEFAULT_GATE, VO.RANK, "linear border"), (VC.zero_dt_case(F), DEFAULT_GATE, VO.RANK, "bias")]
    for F in SINGULAR_FRAMES[1::2]:
        out.append((VC.constant_velocity_case(F), DEFAULT_GATE, VO.RANK, "linear border"))
    out.append((_no_period(VC.make_case(5, 3, 20)), DEFAULT_GATE, VO.RANK, "linear border"))
    out.append((VC.negated_T_case(), DEFAULT_GATE, VO.LINEAR, None))                        # s < 0 in LinearAlignment (:184)
    out.append((VC.huge_acc_case(VC.LINEAR_SIDE_K), DEFAULT_GATE, VO.LINEAR, None))         # | |g| - G | > 1 with |g| ~ 1e206, two decades under the overflow
    out.append((VC.huge_acc_case(VC.NON_FINITE_K), DEFAULT_GATE, VO.NON_FINITE, None))      # s, g of LinearAlignment not finite, two decades over it
    return out


@pytest.fixture(scope="module")
def status_runs(va):
    """every non-OK input aligned alone at its gate: computed once, shared, never changed"""
    return [(c, gate, st, site, va.align([c], va.default_options(min_relative_pivot=gate), want_preint=True)[0]) for c, gate, st, site in _status_inputs()]


def test_every_status_with_its_zero_pattern_and_computed_fields(gpu, va, status_runs):
    seen = set()
    for c, gate, status, site, r in status_runs:
        r64, rld = _reference(gpu, c, r, gate)
        # (NON_FINITE is a verdict about float64's range: long double does not overflow there and says LINEAR, tests/test_vi_alignment_cpu.py)
        assert r64["status"] == status and rld["status"] == (VO.LINEAR if status == VO.NON_FINITE else status), (c["name"], r64["status"], rld["status"])
        assert r["status"] == status, (c["name"], r["status"])
        seen.add((status, r64.get("site")))
        assert r64.get("site") == site, (c["name"], r64.get("site"))
        if site == "bias":      # everything zero, the pre-integrations included
            assert not any(np.asarray(r[k]).any() for k in BITS[1:7] + BITS[8:]), c["name"]
            assert not any(v.any() for v in r["preint"].values()), c["name"]
            assert r["min_pivot"] == 1.0
            continue
        for k in BEHIND[status]:
            assert not np.asarray(r[k]).any() and not np.asarray(r64[k]).any(), (c["name"], k)
        for k in COMPUTED[status]:
            assert np.asarray(r[k]).any(), (c["name"], k)
        assert np.array_equal(r["bg"], c["bg0"] + r["delta_bg"])
        _preint_is_tcv_preintegrate(gpu, c, r)
        _parity(c, r, r64, rld, COMPUTED[status])
        assert 0.5 <= r["min_pivot"] / r64["min_pivot"] <= 2.0, (c["name"], r["min_pivot"], r64["min_pivot"])
        if status == VO.REFINED_SCALE:
            assert r["scale"] < 0
    assert seen == {(VO.LINEAR, None), (VO.REFINED_SCALE, None), (VO.RANK, "bias"), (VO.RANK, "linear border"), (VO.NON_FINITE, None)}


def test_failing_sequences_of_every_kind_in_one_batch_keep_their_solo_bits(va, status_runs):
    oks = [VC.ragged_case(0, 6), VC.vertical_case(4, 10, -1), _no_period(VC.make_case(18, 11, 20))]
    solo_ok = [va.align([c], want_preint=True)[0] for c in oks]
    assert [r["status"] for r in solo_ok] == [0, 0, 0]
    runs = [x for x in status_runs if x[1] == DEFAULT_GATE]
    batch, solo = [], []
    for k, (c, _, _, _, r) in enumerate(runs):
        batch.append(c); solo.append(r)
        if k % 4 == 1:
            batch.append(oks[(k // 4) % 3]); solo.append(solo_ok[(k // 4) % 3])
    assert sum(r["status"] == 0 for r in solo) >= 3
    for c, s, r in zip(batch, solo, va.align(batch, want_preint=True)):
        _same_bits(r, s, c["name"] + " in the mixed batch")
    # the gates of RANK_SITES are options of the call: their own batches, between two sequences that align at that gate too
    for c, gate, _, _, r in [x for x in status_runs if x[1] != DEFAULT_GATE]:
        o = va.default_options(min_relative_pivot=gate)
        nb = [oks[2], c, oks[0]]
        alone = [va.align([oks[2]], o, want_preint=True)[0], r, va.align([oks[0]], o, want_preint=True)[0]]
        assert [a["status"] for a in alone] == [0, VO.RANK, 0]
        for cc, s, b in zip(nb, alone, va.align(nb, o, want_preint=True)):
            _same_bits(b, s, cc["name"] + " at gate %g" % gate)


# ---------------------------------------------------------------------------------------------------------------- host paths
def test_pre_chunk_split_of_a_long_batch(va):
    """the pre-integration passes go in groups of at most 8192 intervals: 64 sequences of 127 intervals and one of 64 end a group at exactly
    8192; the next group stops inside the limit (64 x 127 + 4, then 127 more would pass it); the rest is a third group.  What this checks is
    that every record finds its sequence across three groups.  It can NOT see where a group ends: tcv_preintegrate has no limit of its own and
    the host sizes its buffers per group, so a group one sequence too long gives the same records -- PRE_CHUNK bounds staging memory only."""
    big = va.Sequence(VC.make_case(109, 128, 10, key="one"))
    s65, s5, s5p = va.Sequence(VC.make_case(107, 65, 20, key="sparse")), va.Sequence(VC.make_case(101, 5, 10)), va.Sequence(VC.ragged_case(3, 5))
    S = [big] * 64 + [s65] + [big] * 64 + [s5] + [big] * 2 + [s5p]
    itv = np.cumsum([s.F - 1 for s in S])
    assert itv[64] == 8192 and itv[129] - itv[64] <= 8192 < itv[130] - itv[64] and itv[-1] > 2 * 8192
    want = [False] * (len(S) - 1) + [True]
    solo = {id(s): _align_each(va, [s], [s is s5p])[0] for s in (big, s65, s5, s5p)}
    assert all(r["status"] == 0 for r in solo.values())
    for k, (s, r) in enumerate(zip(S, _align_each(va, S, want))):
        _same_bits(r, solo[id(s)], "sequence %d of the long batch" % k)
    assert "preint" in solo[id(s5p)]


def test_neighbours_with_different_noise_go_into_different_groups(gpu, va):
    base = [_no_period(VC.make_case(200 + k, 5 + k, 10)) for k in range(4)]
    A, B = VC.NOISE, VC.NOISE_B
    cases = [dict(base[0], noise=A), dict(base[0], noise=B), dict(base[1], noise=B), dict(base[2], noise=A), dict(base[3], noise=A)]
    solo = [va.align([c], want_preint=True)[0] for c in cases]
    res = va.align(cases, want_preint=True)
    for c, s, r in zip(cases, solo, res):
        assert r["status"] == 0
        _same_bits(r, s, c["name"])
        _preint_is_tcv_preintegrate(gpu, c, r)      # the covariances are those of the sequence's OWN noise
    assert not np.array_equal(res[0]["preint"]["covariance"], res[1]["preint"]["covariance"])
    for k in BITS:      # and nothing else of the result depends on the noise
        assert np.array_equal(np.asarray(res[0][k]), np.asarray(res[1][k])), k


def test_samples_need_not_be_laid_out_cumulatively(va):
    """`first` is re-based by the host: the intervals in reverse order in samples7, with unused rows (NaN: the validation reads only the rows an
    interval owns) in front, between and behind"""
    c = VC.ragged_case(4, 6)
    s = va.Sequence(c)
    ref = _align_each(va, [s], [True])[0]
    assert ref["status"] == 0
    rows, first, at = [np.full((3, 7), np.nan)], np.zeros(s.F - 1, np.int32), 3
    for i in range(s.F - 2, -1, -1):
        first[i] = at
        rows += [s.samples[s.first[i]:s.first[i] + s.count[i]], np.full((2 + i, 7), np.nan)]
        at += s.count[i] + 2 + i
    samples = np.ascontiguousarray(np.concatenate(rows))
    assert len(samples) == at and not np.array_equal(first, s.first) and (np.diff(first) < 0).all()
    d = va.Desc.from_buffer_copy(s.desc)
    d.first, d.samples7, d.num_samples = va.iptr(first), va.dptr(samples), len(samples)
    rc, res, outs = va.align_raw([d], want_preint=True)
    assert rc == 0
    r = res[0]
    got = dict(status=int(r.status), delta_bg=np.array(r.delta_bg[:]), bg=np.array(r.bg[:]), scale=float(r.scale), gravity_c0=np.array(r.gravity_c0[:]),
               gravity=np.array(r.gravity[:]), rot_diff=np.array(r.rot_diff[:]).reshape(3, 3), min_pivot=float(r.min_pivot), velocity=outs[0].velocity, Ps=outs[0].Ps,
               Rs=outs[0].Rs, Vs=outs[0].Vs, preint=va.preint_dict(outs[0].preint, s.F - 1))
    _same_bits(got, ref, "reversed layout")


def test_the_largest_call(va):
    """TCV_VI_ALIGN_MAX_BATCH sequences in one call, cycled over four sources, one of them singular"""
    src = [va.Sequence(VC.make_case(300, 4, 10)), va.Sequence(VC.stationary_case(5)), va.Sequence(VC.make_case(301, 5, 20, key="one")), va.Sequence(VC.ragged_case(5, 4))]
    solo = [_align_each(va, [s], [False])[0] for s in src]
    assert [r["status"] for r in solo] == [0, VO.RANK, 0, 0]
    n = va.MAX_BATCH
    res = _align_each(va, [src[k % 4] for k in range(n)], [False] * n)
    for k, r in enumerate(res):
        _same_bits(r, solo[k % 4], "sequence %d of %d" % (k, n))


@pytest.mark.parametrize("seed,F", [(0, 6), (1, 23), (2, 65)])
def test_ragged_counts_and_per_sample_dt_inside_a_sequence(gpu, va, seed, F):
    c = VC.ragged_case(seed, F)
    r = va.align([c], want_preint=True)[0]
    assert r["status"] == VO.OK
    _preint_is_tcv_preintegrate(gpu, c, r)
    r64, rld = _reference(gpu, c, r)
    assert r64["status"] == rld["status"] == VO.OK
    _parity(c, r, r64, rld, FAMILIES)
    assert 0.5 <= r["min_pivot"] / r64["min_pivot"] <= 2.0
