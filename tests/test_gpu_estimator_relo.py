"""Relocalisation through the native estimator (include/tcv_estimator_relo.h) on the device.  One stream of 24 frames (14 windows),
max_features = 30, eight fixed iterations, tapped; two requests in the steady state -- before frame 13 for the frame in slot 4, before frame 18
for the frame in slot 9.  match_points are what the matched frame saw in the stream plus 1 / 460 of noise, sorted by id; prev_relo_t / _r is
the stream's true pose of that frame displaced by D = yaw 3 degrees and (0.5, -0.3, 0.1) m.  Every tapped window, relocalisation or not, is
solved again by the NumPy restatement of the reference (oracle/np_oracle.py, tests/relo_oracle.py) with the gates of
tests/test_gpu_estimator_td.py.  The native replays and the oracle's solves are made once per configuration and shared by the tests."""
import functools

import numpy as np
import pytest

import replay
import relo_oracle as RO
import td_oracle as T

pytestmark = pytest.mark.gpu

SEED, SEED_PLAIN, N_FRAMES = 61, 62, 24      # (SEED: chosen on the CPU so that both relocalisation windows get >= 8 factors, asserted below)
F = dict(max_features=30)
REQUESTS = ((13, 4), (18, 9))                # (before frame k, local index)
W = replay.WINDOW_SIZE


@functools.lru_cache(maxsize=None)
def stream(seed):
    return replay.simulate_stream(seed, N_FRAMES, **F)


@functools.lru_cache(maxsize=None)
def untouched():
    import tcv
    return RO.run_native(tcv, [stream(SEED)])[0]


def request(st, serial, frame_index, seed):
    """(serial, match_points, prev_relo_t, prev_relo_r, frame_index) for the stream's frame `serial` (a frame's serial is its index in the stream)"""
    rng = np.random.default_rng(seed)
    pts = st["points"][serial]
    ids = sorted(pts)
    m = np.array([[pts[i][0] + rng.normal() / 460.0, pts[i][1] + rng.normal() / 460.0, float(i)] for i in ids])
    R, t = RO.displaced(st["gt_R"][serial], st["gt_p"][serial])
    return serial, m, t, R, frame_index


@functools.lru_cache(maxsize=None)
def requests():
    """the two requests; the serial in a slot before a frame is read off the untouched run (a request changes no marginalisation flag)"""
    st, out = stream(SEED), {}
    for j, (k, l) in enumerate(REQUESTS):
        nxt, ws, n = untouched()["serials"][k]
        assert nxt == k and n == W and ws[W] == -1
        out[k] = [(0,) + request(st, ws[l], 100 + j, 900 + j)]
    return out


@functools.lru_cache(maxsize=None)
def relo_replay():
    import tcv
    o = RO.run_native(tcv, [stream(SEED)], tap=(0,), relo=requests())[0]
    o["sols"] = RO.solve_windows([w for w, _ in o["wins"]])
    return o


def check_against_oracle(o, what, relo_at=()):
    """check 1: the per-window gates of tests/test_gpu_estimator_td.py, plus relo_pose_out at 1e-6 and the record at 1e-6 / 1e-4 degrees"""
    wins, sols = o["wins"], o["sols"]
    assert len(wins) == N_FRAMES - W and all(r["applied"] == 1 for _, r in wins)
    bad_it, worst = T.compare(wins, sols)
    flags = [r["flag"] for _, r in wins]
    has = [k for k, (w, _) in enumerate(wins) if w.get("relo") is not None]
    assert has == [k - W for k in relo_at], has
    for k in has:
        (w, r), s = wins[k], sols[k]
        assert len(w["relo"]["frame_i"]) >= 8, len(w["relo"]["frame_i"])
        assert r["relo_result"]["valid"] == 1 and np.abs(r["relo"] - w["relo"]["pose"]).max() > 1e-6      # a free block: it moved
        e = dict(relo_pose=np.abs(r["relo"] - s["relo"]).max() / np.abs(s["relo"]).max())
        e.update(RO.record_errors(r["relo_result"], s["relo_result"]))
        for f in RO.MATS:
            e[f] = RO.unit(r["relo_result"][f], s["relo_result"][f])
        for f, v in e.items():
            worst["relo:" + f] = max(v, worst.get("relo:" + f, 0.0))
    print("%s: %d windows (flags %s, relocalisation in %s with %s factors) re-solved by np_oracle: iteration counts differ on %s; worst %s"
          % (what, len(wins), flags, has, [len(wins[k][0]["relo"]["frame_i"]) for k in has], bad_it, {k: float("%.3g" % v) for k, v in worst.items()}))
    assert not bad_it, bad_it
    assert worst["cost"] < 1e-6 and worst["pose"] < 1e-6 and worst["sb"] < 1e-6 and worst["ex"] < 1e-6, worst
    assert worst["lam"] < 1e-5, worst
    for f, v in worst.items():
        if f.startswith("relo:"):
            assert v < (1e-4 if f[5:] in RO.YAWS else 1e-6), (f, worst)
    # check 2: no prior of any window holds a block other than pose, speed-bias or extrinsic
    for w, _ in wins:
        if w["prior"] is not None:
            assert {b[0] for b in w["prior"]["blocks"]} <= {"pose", "sb", "ex"}
            assert sum(w["prior"]["sizes"]) == sum({"pose": 7, "sb": 9, "ex": 7}[b[0]] for b in w["prior"]["blocks"])


def test_every_window_against_the_reference_restatement(gpu):
    o = relo_replay()
    assert o["accepted"] == [(k, 1) for k, _ in REQUESTS]
    for (k, l) in REQUESTS:
        w = o["wins"][k - W][0]["relo"]
        assert w["local_index"] == l and w["frame_serial"] == requests()[k][0][1] and np.all(w["frame_i"] <= l)
    flags = [r["flag"] for _, r in o["wins"]]
    assert replay.MARGIN_OLD in flags
    check_against_oracle(o, "one stream, two requests", [k for k, _ in REQUESTS])


def test_the_correction_points_the_right_way_and_persists(gpu):
    """|drift_correct_r P + drift_correct_t - D(P_true)| < 1/2 |P - D(P_true)| for the position published with the relocalisation frame"""
    o, st = relo_replay(), stream(SEED)
    assert o["relo"][REQUESTS[0][0] - W - 1]["valid"] == 0 and np.array_equal(o["relo"][0]["drift_correct_r"], np.eye(3))
    for j, (k, l) in enumerate(REQUESTS):
        r = o["relo"][k - W]
        assert r["valid"] == 1 and r["frame_index"] == 100 + j and r["frame_serial"] == requests()[k][0][1]
        P = o["p"][k - W]
        _, want = RO.displaced(st["gt_R"][k], st["gt_p"][k])
        before, after = np.linalg.norm(P - want), np.linalg.norm(r["drift_correct_r"] @ P + r["drift_correct_t"] - want)
        print("frame %d: |P - D(P_true)| = %.4f m, corrected %.4f m, drift yaw %.4f deg" % (k, before, after, o["wins"][k - W][1]["relo_result"]["drift_correct_yaw"]))
        assert after < 0.5 * before
        nxt = o["relo"][k - W + 1]      # one frame later: the same record
        assert all(np.array_equal(nxt[f], r[f]) for f in r)


def test_a_request_for_a_frame_outside_the_window_changes_nothing(gpu):
    st = stream(SEED)
    gone = {13: [(0,) + request(st, 0, 7, 5)], 18: [(0, 1000) + request(st, 1, 8, 6)[1:]]}      # serial 0 left the window long ago; 1000 was never given out
    o = RO.run_native(gpu, [st], relo=gone)[0]
    assert o["accepted"] == [(13, 0), (18, 0)]
    for a, b in zip(RO.published(o), RO.published(untouched())):
        assert np.array_equal(a, b)
    assert all(r["valid"] == 0 for r in o["relo"])


@pytest.mark.parametrize("env", [("TCV_EST_HOST_PRIORS", "1"), ("TCV_EST_MARG_DEFER", "1"), ("TCV_EST_HOST_PREINT", "1")])
def test_modes_give_the_same_bits_with_the_two_requests(gpu, monkeypatch, env):
    for k in ("TCV_EST_HOST_PRIORS", "TCV_EST_MARG_DEFER", "TCV_EST_HOST_PREINT"):
        monkeypatch.delenv(k, raising=False)
    want = relo_replay()
    monkeypatch.setenv(*env)
    o = RO.run_native(gpu, [stream(SEED)], tap=(0,), relo=requests())[0]
    for a, b in zip(RO.published(o), RO.published(want)):
        assert np.array_equal(a, b), env
    assert [r["valid"] for r in o["relo"]] == [r["valid"] for r in want["relo"]] and o["relo"][-1]["valid"] == 1
    for ra, rb in zip(o["relo"], want["relo"]):
        assert all(np.array_equal(ra[f], rb[f]) for f in ra), env
    for (wa, ra), (wb, rb) in zip(o["wins"], want["wins"]):
        assert (wa.get("relo") is None) == (wb.get("relo") is None)
        if wa.get("relo") is not None:
            assert np.array_equal(ra["relo"], rb["relo"]) and all(np.array_equal(ra["relo_result"][f], rb["relo_result"][f]) for f in ra["relo_result"])


def test_mixed_lock_step_list_of_a_relocalising_and_a_plain_estimator(gpu):
    """[relo, plain] in one lock-step list, both tapped: both pass the per-window oracle gates (the plain member's frames next to a
    relocalisation window run on another kernel instance: no bit-identity with its solo run is asked for)"""
    a, b = RO.run_native(gpu, [stream(SEED), stream(SEED_PLAIN)], tap=(0, 1), relo=requests())
    sols = RO.solve_windows([w for w, _ in a["wins"]] + [w for w, _ in b["wins"]])
    a["sols"], b["sols"] = sols[:len(a["wins"])], sols[len(a["wins"]):]
    check_against_oracle(a, "relocalising member of the mixed list", [k for k, _ in REQUESTS])
    check_against_oracle(b, "plain member of the mixed list")
    assert all(r["valid"] == 0 for r in b["relo"]) and a["relo"][-1]["valid"] == 1 and b["accepted"] == []
