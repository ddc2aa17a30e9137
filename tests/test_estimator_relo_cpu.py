"""Relocalisation in the native estimator (include/tcv_estimator_relo.h: tcv_estimator_frame_serial, _set_relo_frame, _get_relocalization)
and tcv_problem_set_relocalization (include/tcv.h), host side: begin_frame and the problem graph are host code and run without a GPU."""
import ctypes as C

import numpy as np
import pytest

import replay
import synth
from relo_util import add_relocalisation, hip_relo_window

vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
W = replay.WINDOW_SIZE


@pytest.fixture(scope="module")
def L(built):
    import tcv
    lib = tcv.lib()
    lib.tcv_estimator_create.argtypes = [C.POINTER(vp), C.POINTER(replay._EstimatorConfig)]
    lib.tcv_estimator_destroy.argtypes = [vp]; lib.tcv_estimator_destroy.restype = None
    lib.tcv_estimator_reset.argtypes = [vp]
    lib.tcv_estimator_begin_frame.argtypes = [vp, C.c_int, dp, dp, C.c_int, ip, dp, C.c_int, ip, dp, dp, ip]
    lib.tcv_estimator_finish_frame.argtypes = [vp, dp, dp, dp]
    lib.tcv_estimator_set_time_offset.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.tcv_estimator_frame_serial.argtypes = [vp, ip, ip, ip]
    lib.tcv_estimator_set_relo_frame.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, ip]
    lib.tcv_estimator_get_relocalization.argtypes = [vp, C.POINTER(replay._EstimatorRelo)]
    return lib


def _config():
    cfg = replay._EstimatorConfig()
    cfg.focal_length = 460.0; cfg.min_parallax = replay.MIN_PARALLAX; cfg.init_depth = replay.INIT_DEPTH
    cfg.acc_n = cfg.gyr_n = cfg.acc_w = cfg.gyr_w = 1e-3
    cfg.gravity[:] = [0.0, 0.0, 9.81]; cfg.imu_dt = 0.005; cfg.K[:] = [460.0, 0, 376.0, 0, 460.0, 240.0, 0, 0, 1.0]; cfg.width = 752; cfg.height = 480
    cfg.tic[:] = [0.0, 0.0, 0.0]; cfg.ric[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]; cfg.estimate_extrinsic = 1
    cfg.angle_th, cfg.overlap_th, cfg.dist_th = 0.17, 0.45, 50.0
    cfg.num_iterations = 8
    return cfg


@pytest.fixture
def est(L):
    hs = []

    def make():
        h = vp()
        assert L.tcv_estimator_create(C.byref(h), C.byref(_config())) == 0
        hs.append(h)
        return h
    yield make
    for h in hs:
        L.tcv_estimator_destroy(h)


PTS = np.ascontiguousarray(np.array([[0.1, 0.2, 1.0], [-0.1, 0.05, 1.0]]))
IDS = np.ascontiguousarray([7, 9], dtype=np.int32)
MATCH = np.ascontiguousarray(np.array([[0.11, 0.19, 7.0], [-0.09, 0.06, 9.0]]))
PREV_T = np.ascontiguousarray([0.5, -0.3, 0.1])
PREV_R = np.ascontiguousarray(np.eye(3).reshape(9))


def _begin(L, h):
    r = C.c_int(-1)
    return L.tcv_estimator_begin_frame(h, 0, None, None, 2, IDS.ctypes.data_as(ip), PTS.ctypes.data_as(dp), 0, None, None, None, C.byref(r)), r.value


def _serials(L, h):
    nxt, n = C.c_int(-1), C.c_int(-1)
    ws = (C.c_int * (W + 1))()
    assert L.tcv_estimator_frame_serial(h, C.byref(nxt), ws, C.byref(n)) == 0
    return nxt.value, list(ws), n.value


def _set(L, h, serial, match=MATCH, n=None, prev_t=PREV_T, prev_r=PREV_R, frame_index=17):
    acc = C.c_int(-1)
    rc = L.tcv_estimator_set_relo_frame(h, serial, frame_index, len(match) if n is None else n, None if match is None else match.ctypes.data_as(dp),
                                        None if prev_t is None else prev_t.ctypes.data_as(dp), None if prev_r is None else prev_r.ctypes.data_as(dp), C.byref(acc))
    return rc, acc.value


def _relo(L, h):
    r = replay._EstimatorRelo()
    assert L.tcv_estimator_get_relocalization(h, C.byref(r)) == 0
    return r


def _is_identity_and_zero(r):
    return (r.valid == 0 and list(r.drift_correct_r) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and not any(r.drift_correct_t) and not any(r.relo_relative_t)
            and not any(r.relo_relative_q) and r.relo_relative_yaw == 0.0 and not any(r.relo_r) and not any(r.relo_t))


def test_serials_count_from_zero_and_restart_on_reset(L, est):
    h = est()
    assert _serials(L, h) == (0, [-1] * (W + 1), 0)
    for k in range(4):
        assert _begin(L, h) == (0, 0)
        assert _serials(L, h) == (k + 1, list(range(k + 1)) + [-1] * (W - k), k + 1)
    assert L.tcv_estimator_reset(h) == 0
    assert _serials(L, h) == (0, [-1] * (W + 1), 0)
    assert _begin(L, h) == (0, 0)
    assert _serials(L, h)[:2] == (1, [0] + [-1] * W)
    # any of the three outputs may be left out
    assert L.tcv_estimator_frame_serial(h, None, None, None) == 0
    import tcv
    assert L.tcv_estimator_frame_serial(None, None, None, None) == tcv.TCV_ERR_INVALID


def test_set_relo_frame_while_the_window_fills(L, est):
    """Slots 0 .. WINDOW_SIZE - 1 are searched (estimator.cpp:2269).  Between frames the newest slot -- the one the next begin_frame fills --
    holds no frame yet: its serial-to-be is not found, like a serial that was never given out."""
    h = est()
    for _ in range(3):
        assert _begin(L, h) == (0, 0)
    nxt, ws, n = _serials(L, h)
    assert (nxt, n) == (3, 3) and ws[3] == -1
    for serial in (0, 1, 2):
        assert _set(L, h, serial) == (0, 1)                            # a searched slot
    assert _set(L, h, nxt) == (0, 0)                                   # the newest slot: nothing there yet
    assert _set(L, h, 1000) == (0, 0) and _set(L, h, -1) == (0, 0)     # unknown serials are ignored silently, like the reference does
    assert _set(L, h, 2, match=np.zeros((0, 3)), n=0) == (0, 1)        # an empty match list is a valid request
    # a full window between begin_frame and finish_frame: slot WINDOW_SIZE holds a frame, and the call is refused there (below)
    for _ in range(W - 3):
        assert _begin(L, h) == (0, 0)
    assert _serials(L, h) == (W, list(range(W)) + [-1], W)
    assert _set(L, h, W - 1) == (0, 1) and _set(L, h, W) == (0, 0)


def test_set_relo_frame_rejects_bad_requests(L, est):
    import tcv
    h = est()
    for _ in range(W):
        assert _begin(L, h) == (0, 0)
    bad = [(np.ascontiguousarray(MATCH[::-1]), "ascending"),                                         # unsorted
           (np.ascontiguousarray(np.array([[0.1, 0.2, 7.0], [0.3, 0.1, 7.0]])), "ascending")]        # duplicate id
    for m, word in bad:
        assert _set(L, h, 1, match=m) == (tcv.TCV_ERR_INVALID, 0)
        assert word.encode() in L.tcv_last_error()
    for kw in (dict(match=None, n=2), dict(prev_t=None), dict(prev_r=None), dict(n=-1)):
        assert _set(L, h, 1, **kw) == (tcv.TCV_ERR_INVALID, 0)
        assert len(L.tcv_last_error()) > 0
    assert L.tcv_estimator_set_relo_frame(None, 0, 0, 0, None, PREV_T.ctypes.data_as(dp), PREV_R.ctypes.data_as(dp), C.byref(C.c_int())) == tcv.TCV_ERR_INVALID
    assert _set(L, h, 1) == (0, 1)                                     # ... and the estimator still takes a good one
    # between a begin_frame that reported ready and its finish_frame
    assert _begin(L, h) == (0, 1)
    assert _serials(L, h) == (W + 1, list(range(W + 1)), W + 1)
    assert _set(L, h, 1) == (tcv.TCV_ERR_INVALID, 0)
    assert b"between frames" in L.tcv_last_error()


def test_set_relo_frame_is_refused_with_estimate_td(L, est):
    import tcv
    h = est()
    assert L.tcv_estimator_set_time_offset(h, 1, 0.0, 0.0, 480.0) == 0
    assert _set(L, h, 0) == (tcv.TCV_ERR_INVALID, 0)
    assert b"estimate_td" in L.tcv_last_error()
    g = est()
    assert L.tcv_estimator_set_time_offset(g, 0, 0.0, 0.0, 480.0) == 0      # configured off: a plain estimator
    assert _begin(L, g) == (0, 0)
    assert _set(L, g, 0) == (0, 1)


def test_drift_is_identity_and_zero_before_any_request_and_after_a_reset(L, est):
    h = est()
    assert _is_identity_and_zero(_relo(L, h))
    for _ in range(3):
        assert _begin(L, h) == (0, 0)
    assert _set(L, h, 1) == (0, 1)
    assert _is_identity_and_zero(_relo(L, h))                          # a request alone publishes nothing: only an applied window does
    assert L.tcv_estimator_reset(h) == 0
    assert _is_identity_and_zero(_relo(L, h))
    import tcv
    assert L.tcv_estimator_get_relocalization(h, None) == tcv.TCV_ERR_INVALID


def test_problem_set_relocalization_rejects_its_four_error_cases(built):
    import tcv
    Lb = tcv.lib()
    w = add_relocalisation(dict(synth.window_at(synth.make_windows(9300, 1, with_lines=False), 0), prior=None), f=6, seed=2)
    Wn, relo = hip_relo_window(tcv, w)
    t, r = tcv.f64(PREV_T), tcv.f64(PREV_R)

    def call(p, block, l):
        return Lb.tcv_problem_set_relocalization(p, block, l, tcv.dptr(t), tcv.dptr(r))

    stray = np.zeros(7); stray[6] = 1.0
    assert call(Wn.h, tcv.dptr(stray), 6) == tcv.TCV_ERR_INVALID and b"not a pose block" in Lb.tcv_last_error()            # not a block of the problem
    assert call(Wn.h, Wn.block_ptr("sb", 2), 6) == tcv.TCV_ERR_INVALID and b"not a pose block" in Lb.tcv_last_error()      # a block, but not a 7-dim pose
    assert call(Wn.h, Wn.block_ptr("pose", 3), 6) == tcv.TCV_ERR_INVALID and b"one of the frame poses" in Lb.tcv_last_error()
    for l in (-1, 11):
        assert call(Wn.h, tcv.dptr(relo), l) == tcv.TCV_ERR_INVALID and b"frame_local_index" in Lb.tcv_last_error()
    # no frame table: a problem built block by block, without tcv_problem_set_frames
    p = C.c_void_p()
    assert Lb.tcv_problem_create(C.byref(p)) == 0
    a, b = stray.copy(), stray.copy()
    assert Lb.tcv_problem_add_parameter_block(p, tcv.dptr(a), 7, tcv.TCV_PARAM_POSE) == 0 and Lb.tcv_problem_add_parameter_block(p, tcv.dptr(b), 7, tcv.TCV_PARAM_POSE) == 0
    assert call(p, tcv.dptr(b), 0) == tcv.TCV_ERR_INVALID and b"no frame table" in Lb.tcv_last_error()
    Lb.tcv_problem_destroy(p)
    assert call(Wn.h, tcv.dptr(relo), 6) == 0                          # and the good call
    Wn.set_relocalization(relo, 0, PREV_T, np.eye(3))                  # (the Python wrapper; local index 0 is allowed)
