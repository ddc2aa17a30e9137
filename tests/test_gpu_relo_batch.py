"""The batch path of the relocalisation tail (tcv_problem_set_relocalization, relo_fix_batch_kernel in front of the gauge kernel, the record
riding with the states, tcv_batch_get_relocalization).  Windows: the two of tests/test_gpu_relo.py alone (B = 1), both in a batch of three
with a plain window between them, and every fifth window of a 300-window batch (two workgroups per CU).  Eight fixed iterations, the fused
gauge fix requested and not.

Gates: (1) the states of every window equal, bit for bit, those of the same batch without tcv_problem_set_relocalization gauge-fixed by the
stand-alone kernel; (2) the record equals, bit for bit, tcv_relocalization_fix on the un-fixed states of that twin batch; (3) the record
agrees with tests/relo_oracle.py applied to np_oracle.solve's states at 1e-6 (matrices and vectors, relative to max(1, |.|)) and 1e-4 degrees
(yaw scalars), the states themselves at 1e-6 -- for the 300-window batch on windows 0, 5 and 295 (an oracle solve takes seconds; the other 57
relocalisation windows are held by gates 1 and 2 to the kernel that tests/test_gpu_relo_fix.py gates); (4) valid = 0 on plain windows."""
import functools

import numpy as np
import pytest

import np_oracle as NO
import relo_oracle as RO
import synth
from relo_util import add_relocalisation, hip_relo_window
from util import golden_windows, rel

pytestmark = pytest.mark.gpu

FIG = RO.MATS + ("relo_relative_q",) + RO.YAWS


def with_prev(w, f):
    """prev_relo_t / _r: the matched frame's pose displaced by yaw 3 degrees and (0.5, -0.3, 0.1) m"""
    pose = np.asarray(w["pose"], dtype=float)[f]
    R, t = RO.displaced(NO.q2R(pose[3:]), pose[:3])
    w["relo"].update(local_index=f, prev_relo_t=t, prev_relo_r=R)
    return w


@functools.lru_cache(maxsize=None)
def case(name):
    """the windows of a case: list of window dicts, relocalisation ones carry win["relo"] with local_index and prev_relo_*"""
    pre, main, z = golden_windows()
    a = with_prev(add_relocalisation(main, f=4, seed=1), 4)
    b = with_prev(add_relocalisation(dict(synth.window_at(synth.make_windows(9300, 1, with_lines=False), 0), prior=None), f=6, seed=2), 6)
    if name == "golden":
        return [a]
    if name == "synthetic":
        return [b]
    if name == "three":
        return [a, synth.window_at(synth.make_windows(9301, 1), 0), b]
    batch = synth.make_windows(9400, 300)
    wins = [synth.window_at(batch, k) for k in range(300)]
    for k in range(0, 300, 5):
        f = 3 + (k // 5) % 5
        wins[k] = with_prev(add_relocalisation(dict(wins[k], prior=None), f=f, seed=k), f)
    return wins


ORACLE_WINDOWS = {"golden": [0], "synthetic": [0], "three": [0, 2], "every fifth of 300": [0, 5, 295]}


@functools.lru_cache(maxsize=None)
def oracle():
    """np_oracle's answer to the relocalisation windows gate 3 looks at: solved once, on worker processes, shared by the cases"""
    jobs = [("golden", 0), ("synthetic", 0)] + [("every fifth of 300", k) for k in ORACLE_WINDOWS["every fifth of 300"]]
    sols = RO.solve_windows([case(n)[k] for n, k in jobs])
    out = dict(zip(jobs, sols))
    out[("three", 0)], out[("three", 2)] = out[("golden", 0)], out[("synthetic", 0)]
    return out


def build(gpu, wins, set_relo):
    Ws, relos = [], {}
    for k, w in enumerate(wins):
        if w.get("relo") is None:
            Ws.append(gpu.Window(w))
            continue
        W, relo = hip_relo_window(gpu, w)
        if set_relo:
            W.set_relocalization(relo, w["relo"]["local_index"], w["relo"]["prev_relo_t"], w["relo"]["prev_relo_r"])
        Ws.append(W); relos[k] = relo
    return Ws, relos, gpu.Batch(Ws)


def states(Ws, relos):
    return [(W.pose.copy(), W.sb.copy(), W.ex.copy(), W.lam.copy(), relos[k].copy() if k in relos else None) for k, W in enumerate(Ws)]


@functools.lru_cache(maxsize=None)
def twin(name):
    """the batch without tcv_problem_set_relocalization: its solved states un-fixed, then gauge-fixed by the stand-alone kernel"""
    import tcv as gpu
    wins = case(name)
    Ws, relos, b = build(gpu, wins, False)
    with pytest.raises(gpu.TcvError):
        b.relocalization(0)                                     # nothing downloaded yet
    b.solve(gpu.default_options(8, True)); b.synchronize(); b.download_states()
    raw = states(Ws, relos)
    b.gauge_fix(); b.synchronize(); b.download_states()
    assert all(b.relocalization(k)["valid"] == 0 for k in range(len(wins)))
    return raw, states(Ws, relos)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["golden", "synthetic", "three", "every fifth of 300"])
def test_batch_records_and_states(gpu, name, fused):
    wins = case(name)
    raw, fixed = twin(name)
    Ws, relos, b = build(gpu, wins, True)
    assert sorted(relos) == [k for k, w in enumerate(wins) if w.get("relo") is not None] and len(relos) >= 1
    if name == "every fifth of 300":
        assert b.plan_stats()["lds_bytes"] == 80 * 1024 and len(relos) == 60
    if fused:
        b.fuse_gauge_fix()
    with pytest.raises(gpu.TcvError):
        b.relocalization(0)                                     # TCV_ERR_INVALID before the states have been downloaded
    b.solve(gpu.default_options(8, True)); b.gauge_fix(); b.synchronize(); b.download_states()
    got = states(Ws, relos)
    s = b.summaries()
    # (1) every window's states: the twin's, gauge-fixed by the stand-alone kernel; relo_Pose comes back un-fixed
    for k in range(len(wins)):
        for u, v in zip(got[k], fixed[k]):
            assert (u is None and v is None) or np.array_equal(u, v), k
        if k in relos:
            assert np.array_equal(got[k][4], raw[k][4]) and np.abs(got[k][4] - wins[k]["relo"]["pose"]).max() > 1e-4
    # (2) the record: tcv_relocalization_fix on the twin's un-fixed states
    ks = sorted(relos)
    rl = [wins[k]["relo"] for k in ks]
    want = gpu.relo_fix([NO.q2R(np.asarray(wins[k]["pose"], dtype=float)[0, 3:]) for k in ks], [np.asarray(wins[k]["pose"], dtype=float)[0, :3] for k in ks],
                        [raw[k][0][0] for k in ks], [raw[k][0][r["local_index"]] for k, r in zip(ks, rl)], [raw[k][4] for k in ks],
                        [r["prev_relo_t"] for r in rl], [r["prev_relo_r"] for r in rl])
    recs = {k: b.relocalization(k) for k in range(len(wins))}
    for j, k in enumerate(ks):
        assert recs[k]["valid"] == 1 and s[k].termination != 5
        for f in FIG:
            assert np.array_equal(recs[k][f], want[f][j]), (k, f)
    # (4) plain windows
    assert all(recs[k]["valid"] == 0 and not np.any(recs[k]["relo_r"]) for k in range(len(wins)) if k not in relos)
    # (3) against the restatement on np_oracle's states
    worst = {}
    for k in ORACLE_WINDOWS[name]:
        o = oracle()[(name, k)]
        assert s[k].num_iterations == o["iterations"] and abs(s[k].final_cost - o["cost"]) < 1e-6 * o["cost"]
        e = dict(pose=rel(got[k][0], o["pose"]), sb=rel(got[k][1], o["sb"]), ex=rel(got[k][2], o["ex"]), lam=rel(got[k][3], o["lam"]), relo=rel(got[k][4], o["relo"]))
        e.update(RO.record_errors(recs[k], o["relo_result"]))
        for f in RO.MATS:
            e[f] = RO.unit(recs[k][f], o["relo_result"][f])
        worst = {f: max(v, worst.get(f, 0.0)) for f, v in e.items()}
    print("%s, fused %s: worst against np_oracle %s" % (name, fused, {f: float("%.3g" % v) for f, v in worst.items()}))
    for f in ("pose", "sb", "ex", "lam", "relo") + RO.MATS + ("relo_relative_q",):
        assert worst[f] < 1e-6, (f, worst)
    for f in RO.YAWS:
        assert worst[f] < 1e-4, (f, worst)
