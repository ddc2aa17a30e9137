"""ESTIMATE_TD through the native estimator (include/tcv_estimator.h, tcv_estimator_td.h) on the device: every window of a lock-step replay with
the online camera-IMU time offset -- ProjectionTdFactors on para_Td, para_Td kept in the prior of both marginalisation flavours, td chained
from window to window -- is tapped and solved again by the NumPy restatement of the reference (oracle/np_oracle.py); and an estimator that
does not ask for it is what it was.

One stream of 24 frames (14 windows: MARGIN_OLD and MARGIN_SECOND_NEW), max_features = 30, eight fixed iterations; a second seed for the mixed
lock-step list.  The native replays and the oracle's solves are made once per configuration and shared by the tests."""
import functools

import numpy as np
import pytest

import replay
import td_oracle as T

pytestmark = pytest.mark.gpu

SEED, SEED_PLAIN, N_FRAMES, TD_TRUE = 61, 62, 24, 0.004
F = dict(max_features=30)


@functools.lru_cache(maxsize=None)
def td_stream(TR):
    return replay.simulate_stream_td(SEED, N_FRAMES, TD_TRUE, TR=TR, **F)


@functools.lru_cache(maxsize=None)
def plain_stream(seed):
    return replay.simulate_stream(seed, N_FRAMES, **F)


@functools.lru_cache(maxsize=None)
def td_replay(TR):
    """the TD stream alone, tapped, and the oracle's answer to each of its windows"""
    import tcv
    o = T.run_native(tcv, [td_stream(TR)], tap=(0,), estimate_td=True, td0=0.0, TR=TR)[0]
    o["sols"] = T.solve_windows([w for w, _ in o["wins"]])
    return o


@functools.lru_cache(maxsize=None)
def plain_solo():
    import tcv
    return T.run_native(tcv, [plain_stream(SEED_PLAIN)])[0]


def check_against_oracle(o, what):
    """check 1 of the issue on a tapped TD replay: the project's own gates, window by window"""
    wins, sols = o["wins"], o["sols"]
    assert len(wins) == N_FRAMES - replay.WINDOW_SIZE and all(r["applied"] == 1 for _, r in wins)
    bad_it, worst = T.compare(wins, sols)
    flags = [r["flag"] for _, r in wins]
    print("%s: %d windows (flags %s) re-solved by np_oracle: iteration counts differ on %s; worst %s"
          % (what, len(wins), flags, bad_it, {k: float("%.3g" % v) for k, v in worst.items()}))
    assert replay.MARGIN_OLD in flags and replay.MARGIN_SECOND_NEW in flags
    assert not bad_it, bad_it
    assert worst["cost"] < 1e-6 and worst["pose"] < 1e-6 and worst["sb"] < 1e-6 and worst["ex"] < 1e-6, worst
    assert worst["lam"] < 1e-5, worst
    assert worst["td"] < 1e-6, worst                       # |td - td_oracle| < 1e-6 max(1e-3, |td_oracle|)  (tests/test_gpu_td.py:44-45)
    # para_Td in the chained prior: from the second MARGIN_OLD window on (the first one's marginalisation put it there, both flavours keep it)
    old = [k for k, f in enumerate(flags) if f == replay.MARGIN_OLD]
    for k in range(old[1], len(wins)):
        pr = wins[k][0]["prior"]
        assert pr is not None
        at = [i for i, b in enumerate(pr["blocks"]) if b[0] == "td"]
        assert len(at) == 1 and tuple(pr["blocks"][at[0]]) == ("td", 0) and pr["sizes"][at[0]] == 1, (k, pr["blocks"])
    # the chain itself: a window starts from the td its predecessor left, stamps included (cur_td of an observation = td when it was added)
    for k in range(1, len(wins)):
        assert wins[k][0]["td"] == wins[k - 1][1]["td"] == o["td"][k - 1]
        assert set(np.unique(np.concatenate([wins[k][0]["proj"]["td_i"], wins[k][0]["proj"]["td_j"]]))) <= {0.0} | set(o["td"][:k])


@pytest.mark.parametrize("TR", [0.0, 0.02])
def test_every_window_against_the_reference_restatement(gpu, TR):
    o = td_replay(TR)
    assert all(w["proj"]["TR"] == TR and w["proj"]["ROW"] == 480.0 and w.get("td") is not None for w, _ in o["wins"])
    check_against_oracle(o, "TR = %g" % TR)


def test_td_moves_towards_the_true_offset(gpu):
    """td_true = 4 ms, td0 = 0: the first applied window moves td, the last one has halved the distance.  By the test above the restated
    reference gives the same td, window by window (profiles/estimator_td.txt lists both)."""
    o = td_replay(0.0)
    td = o["td"]
    print("td per window [ms]: native %s, oracle %s" % (["%.3f" % (1e3 * v) for v in td], ["%.3f" % (1e3 * s["td"]) for s in o["sols"]]))
    assert td[0] != 0.0
    assert abs(td[-1] - TD_TRUE) < abs(0.0 - TD_TRUE) / 2


def test_no_behaviour_change_without_estimate_td(gpu):
    """the same plain stream untouched, with point aux staged while estimate_td is off, and after tcv_estimator_set_time_offset(e, 0, ...):
    every published state and every per-window statistic bit for bit"""
    st = plain_stream(SEED_PLAIN)
    z = replay.simulate_stream_td(SEED_PLAIN, N_FRAMES, 0.0, **F)      # (td_true = 0, TR = 0: the points are the plain stream's, plus their aux)
    assert all(np.array_equal(z["points"][k][i], p) for k in range(N_FRAMES) for i, p in st["points"][k].items())
    want = T.published(plain_solo())
    staged = T.run_native(gpu, [z])[0]
    off = T.run_native(gpu, [st], estimate_td=False, td0=0.003, TR=0.02)[0]
    staged_off = T.run_native(gpu, [z], estimate_td=False, td0=0.003, TR=0.02)[0]
    assert len(want[1]) == N_FRAMES - replay.WINDOW_SIZE
    for name, o in (("aux staged", staged), ("set_time_offset(0)", off), ("both", staged_off)):
        got = T.published(o)
        assert len(got) == len(want)
        for a, b in zip(got[:4] + got[5:], want[:4] + want[5:]):
            assert np.array_equal(a, b), name
    assert not np.any(T.published(staged)[4]) and np.all(T.published(off)[4] == 0.003)      # td: never configured 0, configured off: td0, untouched by the windows


@pytest.mark.parametrize("env", [("TCV_EST_HOST_PRIORS", "1"), ("TCV_EST_MARG_DEFER", "1"), ("TCV_EST_HOST_PREINT", "1")])
def test_modes_give_the_same_bits_with_estimate_td(gpu, monkeypatch, env):
    """host priors, deferred marginalisation and host pre-integration against the default path (device-resident prior and pre-integrations,
    eager marginalisation), ESTIMATE_TD on with the rolling-shutter term"""
    for k in ("TCV_EST_HOST_PRIORS", "TCV_EST_MARG_DEFER", "TCV_EST_HOST_PREINT"):
        monkeypatch.delenv(k, raising=False)
    want = T.published(td_replay(0.02))
    monkeypatch.setenv(*env)
    o = T.run_native(gpu, [td_stream(0.02)], tap=(0,), estimate_td=True, td0=0.0, TR=0.02)[0]
    got = T.published(o)
    assert len(got) == len(want) and np.any(got[4])
    for a, b in zip(got, want):
        assert np.array_equal(a, b), env
    kept = [sum(b[0] == "td" for b in (w["prior"] or {"blocks": []})["blocks"]) for w, _ in o["wins"]]
    assert kept[0] == 0 and set(kept[2:]) == {1}, kept


def test_mixed_lock_step_list_of_a_td_and_a_plain_estimator(gpu):
    """[TD, plain] in one lock-step list: the TD member passes the per-window oracle gates; the plain member equals its solo run bit for
    bit (a plain stream gives the same bits alone and beside another plain stream at the parent commit: profiles/estimator_td.txt)"""
    td_o, plain_o = T.run_native(gpu, [td_stream(0.02), plain_stream(SEED_PLAIN)], tap=(0,), estimate_td=[True, None], td0=0.0, TR=0.02)
    td_o["sols"] = T.solve_windows([w for w, _ in td_o["wins"]])
    check_against_oracle(td_o, "TD member of the mixed list")
    assert not np.any(plain_o["td"])
    for a, b in zip(T.published(plain_o), T.published(plain_solo())):
        assert np.array_equal(a, b)
