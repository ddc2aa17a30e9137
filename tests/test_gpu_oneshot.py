"""The one-shot entry points that share one round-trip guard (csrc/tcv_runtime.h RoundTrip): the five factor evaluators, tcv_gauge_fix,
tcv_relocalization_fix and tcv_pose_graph_eval_edges.  Each uploads a few arrays, launches one small kernel and fetches the result through
one pinned staging buffer [inputs | outputs] and one pooled device buffer [inputs | outputs | scratch] on the calling thread's stream.

Two properties, both bit for bit (the numbers themselves are gated in test_gpu_factors / _gauge / _relo_fix / _pose_graph):
  size independence    item i of a call with n items is item i of the call with 257 items, for n on both sides of the 64- and 256-wide
                       blocks; odd n also shifts where the regions of the two buffers meet.  Residuals without the optional Jacobian are the
                       residuals with it.
  thread independence  four host threads call the same entry point at once, eight rounds each, every call with its own inputs: each
                       result is the result of the same call made alone.  A staging or device buffer shared between calls would show here.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_MAX = 257
SIZES = (1, 63, 64, 65, 257)
THREADS, ROUNDS, N_THREAD_CALL = 4, 8, 96      # call (t, r) takes items [5 (8 t + r), 5 (8 t + r) + 96) of the 257


def _quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _pose(rng, n):
    return np.concatenate([rng.uniform(-2, 2, (n, 3)), _quat(rng, n)], 1)


def _rot(rng, n):
    """n proper rotation matrices"""
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.linalg.det(q))[:, None, None]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    assert len(got) == len(want)
    return all(g.shape == w.shape and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


# ---- the eight entry points: make(rng) -> inputs over N_MAX items; call(tcv, pg, inputs, rows, jac) -> arrays with one row per item
def _make_imu(rng):
    n = N_MAX
    A = rng.normal(size=(n, 15, 15)) * 1e-3
    return dict(pre=dict(frame_i=np.zeros(n, int), delta_p=rng.normal(size=(n, 3)), delta_q=_quat(rng, n), delta_v=rng.normal(size=(n, 3)),
                         lin_ba=rng.normal(size=(n, 3)) * 0.1, lin_bg=rng.normal(size=(n, 3)) * 0.01, sum_dt=rng.uniform(0.05, 0.5, n),
                         jacobian=rng.normal(size=(n, 15, 15)) * 0.1, covariance=A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(15)),
                params=np.concatenate([_pose(rng, n), rng.normal(size=(n, 9)), _pose(rng, n), rng.normal(size=(n, 9))], 1),
                G=np.array([0.0, 0.0, 9.81]))


def _call_imu(tcv, pg, d, rows, jac=True):
    if "packed" not in d:      # (the ctypes records once: they are the slow part of tcv.eval_imu)
        d["packed"] = np.frombuffer(tcv.pack_imu(d["pre"]), dtype=np.uint8).reshape(N_MAX, -1).copy()
    n = len(rows)
    pre = (tcv.ImuPreintegration * n).from_buffer_copy(np.ascontiguousarray(d["packed"][rows]).tobytes())
    params = np.ascontiguousarray(d["params"][rows])
    S = np.zeros((n, 225)); res = np.zeros((n, 15)); J = np.zeros((n, 480))      # use_given = 0: sqrt_info is made on the device and comes back
    tcv.check(tcv.lib().tcv_eval_imu_factors(n, pre, tcv.dptr(params), tcv.dptr(d["G"]), 0, tcv.dptr(S), tcv.dptr(res), tcv.dptr(J) if jac else None))
    return (res, S, J) if jac else (res, S)


def _make_proj(rng):
    n = N_MAX
    return dict(pts=np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.ones((n, 1)), rng.uniform(-0.5, 0.5, (n, 2)), np.ones((n, 1))], 1),
                aux=rng.normal(size=(n, 8)) * 0.01,
                params=np.concatenate([_pose(rng, n), _pose(rng, n), _pose(rng, n) * 0.1, rng.uniform(0.2, 1.0, (n, 1)), rng.normal(size=(n, 1)) * 0.01], 1))


def _call_proj(tcv, pg, d, rows, jac=True):
    r, Js = tcv.eval_proj(d["pts"][rows], np.ascontiguousarray(d["params"][rows, :22]), 230.0, want_jac=jac)
    return (r, *Js) if jac else (r,)


def _call_proj_td(tcv, pg, d, rows, jac=True):
    r, Js = tcv.eval_proj_td(d["pts"][rows], d["aux"][rows], d["params"][rows], 230.0, 0.03, 480.0, want_jac=jac)
    return (r, *Js) if jac else (r,)


def _make_line(rng):
    n = N_MAX
    K = np.array([[460.0, 0, 376], [0, 460.0, 240], [0, 0, 1]])
    return dict(line=np.concatenate([rng.uniform(-3, 3, (n, 6)), rng.normal(size=(n, 3))], 1), K=K, R=_rot(rng, 1)[0], T=rng.normal(size=3) * 0.1,
                pose=_pose(rng, n))


def _call_line(tcv, pg, d, rows, jac=True):
    r, J = tcv.eval_line(d["line"][rows], d["K"], d["R"], d["T"], d["pose"][rows], want_jac=jac)
    return (r, J) if jac else (r,)


def _make_plus(rng):
    return dict(x=_pose(rng, N_MAX), delta=rng.normal(size=(N_MAX, 6)) * 0.1)


def _call_plus(tcv, pg, d, rows, jac=True):
    return (tcv.pose_plus(d["x"][rows], d["delta"][rows]),)


def _make_gauge(rng):
    return dict(R0=_rot(rng, 1)[0], P0=rng.normal(size=3), pose=_pose(rng, N_MAX), sb=rng.normal(size=(N_MAX, 9)))


def _call_gauge(tcv, pg, d, rows, jac=True):      # (every frame is fixed against frame 0 of ITS call: prefixes share it)
    return tcv.gauge_fix(d["R0"], d["P0"], d["pose"][rows], d["sb"][rows])


def _make_relo(rng):
    n = N_MAX
    return dict(a=[_rot(rng, n), rng.normal(size=(n, 3)), _pose(rng, n), _pose(rng, n), _pose(rng, n), rng.normal(size=(n, 3)), _rot(rng, n)])


def _call_relo(tcv, pg, d, rows, jac=True):
    out = tcv.relo_fix(*[x[rows] for x in d["a"]])
    assert np.all(out["valid"] == 1)
    return tuple(np.asarray(out[k], dtype=np.float64) for k in sorted(out) if k != "valid")


def _make_edges(rng):
    n = N_MAX
    return dict(kind=rng.integers(0, 2, n), yaw_i=rng.uniform(-180, 180, n), t_i=rng.normal(size=(n, 3)), yaw_j=rng.uniform(-180, 180, n),
                t_j=rng.normal(size=(n, 3)), meas=np.concatenate([rng.normal(size=(n, 3)), rng.uniform(-180, 180, (n, 1)), rng.uniform(-20, 20, (n, 2))], 1))


def _call_edges(tcv, pg, d, rows, jac=True):      # (n ints in front of the outputs: an odd n moves their 8-byte alignment)
    return pg.eval_edges(d["kind"][rows], d["yaw_i"][rows], d["t_i"][rows], d["yaw_j"][rows], d["t_j"][rows], d["meas"][rows])


ENTRY = dict(eval_imu=(_make_imu, _call_imu, True), eval_proj=(_make_proj, _call_proj, True), eval_proj_td=(_make_proj, _call_proj_td, True),
             eval_line=(_make_line, _call_line, True), pose_plus=(_make_plus, _call_plus, False), gauge_fix=(_make_gauge, _call_gauge, False),
             relo_fix=(_make_relo, _call_relo, False), pose_graph_eval_edges=(_make_edges, _call_edges, False))


@pytest.fixture(scope="module")
def pg(gpu):
    import tcv_pose_graph
    return tcv_pose_graph


@pytest.fixture(scope="module")
def cases(gpu, pg):
    """per entry point: its seeded inputs and the result of the call with all 257 items, computed once and left alone"""
    out = {}
    for k, (name, (make, call, _)) in enumerate(sorted(ENTRY.items())):
        d = make(np.random.Generator(np.random.PCG64(7100 + k)))
        out[name] = (d, call(gpu, pg, d, np.arange(N_MAX)))
    return out


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_result_of_an_item_does_not_depend_on_the_size_of_the_call(gpu, pg, cases, name):
    d, ref = cases[name]
    call, has_jac = ENTRY[name][1], ENTRY[name][2]
    assert all(np.all(np.isfinite(a)) for a in ref)
    for n in SIZES:
        rows = np.arange(n)
        got = call(gpu, pg, d, rows)
        assert _same(got, [a[:n] for a in ref]), (name, n)
        if has_jac:      # the optional Jacobian left out: the other outputs keep their bits
            bare = call(gpu, pg, d, rows, jac=False)
            assert _same(bare, [a[:n] for a in ref[:len(bare)]]), (name, n, "no Jacobian")


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_concurrent_calls_from_four_threads_match_the_same_calls_made_alone(gpu, pg, cases, name):
    d = cases[name][0]
    call = ENTRY[name][1]
    rows = {(t, r): np.arange(N_THREAD_CALL) + 5 * (ROUNDS * t + r) for t in range(THREADS) for r in range(ROUNDS)}
    assert max(v[-1] for v in rows.values()) < N_MAX and len({v[0] for v in rows.values()}) == THREADS * ROUNDS
    alone = {k: call(gpu, pg, d, v) for k, v in rows.items()}      # on the main thread, one after the other
    got, errors, gate = {}, [], threading.Barrier(THREADS)

    def worker(t):
        try:
            gate.wait()
            for r in range(ROUNDS):
                got[(t, r)] = call(gpu, pg, d, rows[(t, r)])
        except BaseException as e:      # noqa: BLE001  (reported by the main thread)
            errors.append((t, repr(e)))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in rows:
        assert _same(got[k], alone[k]), (name, "thread %d round %d" % k)
