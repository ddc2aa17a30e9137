"""tcv_relocalization_fix (relo_fix_kernel, csrc/tcv_relo.hip): the tail of Estimator::double2vector (estimator.cpp:1606-1624) on seeded random
cases against its NumPy restatement (tests/relo_oracle.py).  Case kinds of tests/dev/fuzz_gauge.py for Rs[0] / para_Pose[0]: free, singular R0,
singular pose 0, band edge (89 degrees +- 1e-6 / 1e-3), yaw +-179.9; relo_Pose, para_Pose[l] and prev_relo_r with |pitch| <= 80 degrees.

Gates: the project's gauge gate of 1e-12 on relo_r, relo_t, relo_relative_t and on relo_relative_q as a rotation;
1e-10 relative to max(1, |.|) on drift_correct_r / _t; 1e-9 degrees, modulo 360, on the two yaw scalars (their conditioning: 1 / cos 80 degrees
times translations of ~20 m, on top of the 57 x a pose 0 at 89 degrees pitch puts on y_diff).  Measured worst values: profiles/estimator_relo.txt."""
import functools

import numpy as np
import pytest

import np_oracle as NO
import relo_oracle as RO

pytestmark = pytest.mark.gpu

N_CASES = 2000
KINDS = ("free", "singular R0", "singular pose0", "band edge", "yaw 180")
KEYS = ("R0", "P0", "pose0", "pose_l", "relo_pose", "prev_relo_t", "prev_relo_r")


def rand_R(rng, pitch=None, yaw=None, max_pitch=89.0):
    y = rng.uniform(-180, 180) if yaw is None else yaw
    p = rng.uniform(-max_pitch, max_pitch) if pitch is None else pitch
    return NO.ypr2R(np.array([y, p, rng.uniform(-180, 180)]))


def rand_pose(rng, R):
    q = NO.R2q(R)
    return np.concatenate([rng.normal(size=3) * 5, q / np.linalg.norm(q)])


@functools.lru_cache(maxsize=None)
def cases():
    """the inputs (arrays over the cases), the case kinds and the restatement's records: made once, shared by the tests"""
    a = {k: [] for k in KEYS}
    kinds, ref = [], []
    for c in range(N_CASES):
        rng = np.random.default_rng(730000 + c)
        kind = KINDS[c % len(KINDS)]
        p0 = p00 = y0 = y00 = None
        if kind == "singular R0":
            p0 = float(rng.choice([-1, 1])) * rng.uniform(89.2, 89.99)
        elif kind == "singular pose0":
            p00 = float(rng.choice([-1, 1])) * rng.uniform(89.2, 89.99)
        elif kind == "band edge":
            edge = float(rng.choice([-1, 1])) * (89.0 + float(rng.choice([-1e-3, -1e-6, 1e-6, 1e-3])))
            if rng.integers(2):
                p0 = edge
            else:
                p00 = edge
        elif kind == "yaw 180":
            y0, y00 = 179.9, -179.9
        one = dict(R0=rand_R(rng, p0, y0), P0=rng.normal(size=3) * 5, pose0=rand_pose(rng, rand_R(rng, p00, y00)), pose_l=rand_pose(rng, rand_R(rng, max_pitch=80.0)),
                   relo_pose=rand_pose(rng, rand_R(rng, max_pitch=80.0)), prev_relo_t=rng.normal(size=3) * 5, prev_relo_r=rand_R(rng, max_pitch=80.0))
        for k in KEYS:
            a[k].append(one[k])
        kinds.append(kind)
        ref.append(RO.relo_tail(**one))
    return {k: np.array(v) for k, v in a.items()}, kinds, ref


def record(out, i):
    return {k: out[k][i] for k in RO.MATS + ("relo_relative_q",) + RO.YAWS}


def check(out, ref, kinds, idx):
    worst = {}
    for j, i in enumerate(idx):
        e = RO.record_errors(record(out, j), ref[i])
        for k, v in e.items():
            if v > worst.get((kinds[i], k), (0.0, -1))[0]:
                worst[(kinds[i], k)] = (v, i)
    by_key = {}
    for (kind, k), (v, i) in worst.items():
        if v > by_key.get(k, (0.0, "", -1))[0]:
            by_key[k] = (v, kind, i)
    print("worst per figure (value, kind, case):", {k: ("%.2e" % v, kind, i) for k, (v, kind, i) in sorted(by_key.items())})
    assert all(out["valid"] == 1)
    for k in ("relo_r", "relo_t", "relo_relative_t", "relo_relative_q"):
        assert by_key.get(k, (0.0,))[0] < 1e-12, (k, by_key[k])
    for k in ("drift_correct_r", "drift_correct_t"):
        assert by_key.get(k, (0.0,))[0] < 1e-10, (k, by_key[k])
    for k in RO.YAWS:
        assert by_key.get(k, (0.0,))[0] < 1e-9, (k, by_key[k])


def test_2000_seeded_cases_against_the_restatement(gpu):
    a, kinds, ref = cases()
    assert {k: kinds.count(k) for k in KINDS} == {k: N_CASES // len(KINDS) for k in KINDS}
    out = gpu.relo_fix(*[a[k] for k in KEYS])
    check(out, ref, kinds, range(N_CASES))


def test_one_case_and_the_largest_call(gpu):
    """n = 1, and n = 4096 (the largest call, 64 workgroups): every case gives what it gives in the call of 2000, bit for bit"""
    a, kinds, ref = cases()
    base = gpu.relo_fix(*[a[k] for k in KEYS])
    one = gpu.relo_fix(*[a[k][7:8] for k in KEYS])
    check(one, ref, kinds, [7])
    idx = np.arange(4096) % N_CASES
    big = gpu.relo_fix(*[a[k][idx] for k in KEYS])
    check(big, ref, kinds, idx)
    for k in RO.MATS + ("relo_relative_q",) + RO.YAWS:
        assert np.array_equal(one[k][0], base[k][7]), k
        assert np.array_equal(big[k], base[k][idx]), k
    with pytest.raises(gpu.TcvError):
        gpu.relo_fix(*[a[k][np.arange(4097) % N_CASES] for k in KEYS])
    bad = a["relo_pose"][:3].copy(); bad[1, 4] = np.nan
    with pytest.raises(gpu.TcvError):
        gpu.relo_fix(*[bad if k == "relo_pose" else a[k][:3] for k in KEYS])
