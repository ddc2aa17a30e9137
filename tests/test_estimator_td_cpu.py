"""ESTIMATE_TD in the native estimator (include/tcv_estimator.h: tcv_estimator_set_time_offset, _stage_point_aux, _get_time_offset), host side:
begin_frame is host code and runs without a GPU, like tests/test_replay_cpu.py::test_native_estimator_host_side_entry_points_without_a_device."""
import ctypes as C

import numpy as np
import pytest

import replay

vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def L(built):
    import tcv
    lib = tcv.lib()
    lib.tcv_estimator_create.argtypes = [C.POINTER(vp), C.POINTER(replay._EstimatorConfig)]
    lib.tcv_estimator_destroy.argtypes = [vp]; lib.tcv_estimator_destroy.restype = None
    lib.tcv_estimator_reset.argtypes = [vp]
    lib.tcv_estimator_begin_frame.argtypes = [vp, C.c_int, dp, dp, C.c_int, ip, dp, C.c_int, ip, dp, dp, ip]
    lib.tcv_estimators_begin_frames.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(replay._FrameInput), ip, ip]
    lib.tcv_estimator_set_time_offset.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.tcv_estimator_stage_point_aux.argtypes = [vp, C.c_int, dp]
    lib.tcv_estimator_get_time_offset.argtypes = [vp, dp]
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
AUX = np.ascontiguousarray(np.array([[422.0, 332.0, 0.3, -0.1], [330.0, 263.0, 0.0, 0.2]]))


def _begin(L, h, n_points=2):
    r = C.c_int(-1)
    return L.tcv_estimator_begin_frame(h, 0, None, None, n_points, IDS.ctypes.data_as(ip), PTS.ctypes.data_as(dp), 0, None, None, None, C.byref(r)), r.value


def _td(L, h):
    td = C.c_double(-1.0)
    assert L.tcv_estimator_get_time_offset(h, C.byref(td)) == 0
    return td.value


def test_time_offset_starts_at_td0_and_returns_to_it_on_reset(L, est):
    h = est()
    assert _td(L, h) == 0.0                                            # never configured: TD = 0
    assert L.tcv_estimator_set_time_offset(h, 1, 0.0125, 0.033, 480.0) == 0
    assert _td(L, h) == 0.0125
    assert L.tcv_estimator_stage_point_aux(h, 2, AUX.ctypes.data_as(dp)) == 0
    assert _begin(L, h) == (0, 0)
    assert _td(L, h) == 0.0125
    assert L.tcv_estimator_reset(h) == 0
    assert _td(L, h) == 0.0125                                         # `td = TD` (estimator.cpp:51, :170); the setting survives the reset
    assert L.tcv_estimator_set_time_offset(h, 1, -0.002, 0.0, 480.0) == 0      # allowed again: the window is empty
    assert _td(L, h) == -0.002
    # the reset estimator still asks for the aux of its frames
    import tcv
    rc, _ = _begin(L, h)
    assert rc == tcv.TCV_ERR_INVALID and b"no point aux" in L.tcv_last_error()


def test_set_time_offset_is_refused_once_a_frame_is_in_the_window(L, est):
    import tcv
    h = est()
    assert _begin(L, h) == (0, 0)
    assert L.tcv_estimator_set_time_offset(h, 1, 0.0, 0.0, 480.0) == tcv.TCV_ERR_INVALID
    assert b"window is empty" in L.tcv_last_error()
    assert _td(L, h) == 0.0
    assert _begin(L, h) == (0, 0)                                      # and it stayed a plain estimator: no aux wanted


@pytest.mark.parametrize("ROW", [0.0, -480.0, float("nan")])
@pytest.mark.parametrize("on", [0, 1])
def test_row_must_be_positive(L, est, on, ROW):
    import tcv
    h = est()
    assert L.tcv_estimator_set_time_offset(h, on, 0.0, 0.0, ROW) == tcv.TCV_ERR_INVALID
    assert b"ROW" in L.tcv_last_error()
    assert L.tcv_estimator_set_time_offset(None, on, 0.0, 0.0, 480.0) == tcv.TCV_ERR_INVALID


def test_missing_and_miscounted_aux_fail_begin_frame(L, est):
    import tcv
    h = est()
    assert L.tcv_estimator_set_time_offset(h, 1, 0.0, 0.0, 480.0) == 0
    rc, _ = _begin(L, h)                                               # nothing staged
    assert rc == tcv.TCV_ERR_INVALID and b"staged" in L.tcv_last_error()
    assert L.tcv_estimator_stage_point_aux(h, 1, AUX.ctypes.data_as(dp)) == 0
    rc, _ = _begin(L, h)                                               # one point staged, two in the frame
    assert rc == tcv.TCV_ERR_INVALID and b"1 points were staged" in L.tcv_last_error()
    rc, _ = _begin(L, h)                                               # the failed call consumed it
    assert rc == tcv.TCV_ERR_INVALID and b"no point aux" in L.tcv_last_error()
    assert L.tcv_estimator_stage_point_aux(h, 2, AUX.ctypes.data_as(dp)) == 0
    assert _begin(L, h) == (0, 0)
    rc, _ = _begin(L, h)                                               # consumed by the frame it was staged for
    assert rc == tcv.TCV_ERR_INVALID
    # the failed calls left the window alone: ten more frames fill it, the eleventh overall is ready
    ready = []
    for _ in range(10):
        assert L.tcv_estimator_stage_point_aux(h, 2, AUX.ctypes.data_as(dp)) == 0
        rc, r = _begin(L, h)
        assert rc == 0
        ready.append(r)
    assert ready == [0] * 9 + [1]
    assert L.tcv_estimator_stage_point_aux(h, -1, None) == tcv.TCV_ERR_INVALID
    assert L.tcv_estimator_stage_point_aux(h, 2, None) == tcv.TCV_ERR_INVALID
    assert L.tcv_estimator_stage_point_aux(h, 0, None) == 0           # a frame without points stages none


def test_batched_begin_frames_reports_the_aux_errors_per_estimator(L, est):
    import tcv
    hs = [est() for _ in range(4)]                                     # TD without aux | TD with a wrong count | TD staged right | plain
    for h in hs[:3]:
        assert L.tcv_estimator_set_time_offset(h, 1, 0.0, 0.02, 480.0) == 0
    assert L.tcv_estimator_stage_point_aux(hs[1], 1, AUX.ctypes.data_as(dp)) == 0
    assert L.tcv_estimator_stage_point_aux(hs[2], 2, AUX.ctypes.data_as(dp)) == 0
    rec = (replay._FrameInput * 4)()
    for r in rec:
        r.n_imu = 0; r.n_points = 2; r.point_ids = IDS.ctypes.data_as(ip); r.points = PTS.ctypes.data_as(dp); r.n_lines = 0
    ready = (C.c_int * 4)(5, 5, 5, 5); rcs = (C.c_int * 4)(9, 9, 9, 9)
    assert L.tcv_estimators_begin_frames((vp * 4)(*hs), 4, rec, ready, rcs) == tcv.TCV_ERR_INVALID
    assert L.tcv_last_error() and b"no point aux" in L.tcv_last_error()           # the first failure's text
    assert list(rcs) == [tcv.TCV_ERR_INVALID, tcv.TCV_ERR_INVALID, 0, 0] and list(ready) == [0, 0, 0, 0]
    # the two that failed took no frame: staged properly they take their first one now, next to the others' second
    for h in hs[:3]:
        assert L.tcv_estimator_stage_point_aux(h, 2, AUX.ctypes.data_as(dp)) == 0
    assert L.tcv_estimators_begin_frames((vp * 4)(*hs), 4, rec, ready, rcs) == 0 and list(rcs) == [0, 0, 0, 0]
    only = (C.c_int * 1)(9)
    assert L.tcv_estimators_begin_frames((vp * 1)(hs[1]), 1, rec, ready, only) == tcv.TCV_ERR_INVALID and only[0] == tcv.TCV_ERR_INVALID
    assert b"no point aux" in L.tcv_last_error()


@pytest.mark.parametrize("configured", [False, True])
def test_staged_aux_is_accepted_and_dropped_with_estimate_td_off(L, est, configured):
    h = est()
    if configured:
        assert L.tcv_estimator_set_time_offset(h, 0, 0.003, 0.02, 480.0) == 0
    assert L.tcv_estimator_stage_point_aux(h, 1, AUX.ctypes.data_as(dp)) == 0      # (not even the count matters)
    assert _begin(L, h) == (0, 0)
    assert _begin(L, h) == (0, 0)
    assert _td(L, h) == (0.003 if configured else 0.0)


def test_simulate_stream_td_wraps_the_plain_stream():
    """same draws as simulate_stream; velocities are the tracker's finite differences; the shift is with_time_offset's construction"""
    import synth
    kw = dict(max_features=12, max_lines=2)
    st0 = replay.simulate_stream(3, 5, **kw)
    st = replay.simulate_stream_td(3, 5, 0.004, TR=0.02, **kw)
    assert st["td_true"] == 0.004 and st["TR"] == 0.02 and st["ROW"] == float(synth.IMG_H)
    for k in ("t", "gt_p", "gt_R", "gt_v", "ba", "bg"):
        assert np.array_equal(st[k], st0[k])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(st["imu"][1:], st0["imu"][1:]))
    seen_old = 0
    for k in range(5):
        assert list(st["points"][k]) == list(st0["points"][k]) == list(st["point_aux"][k])
        for i, p0 in st0["points"][k].items():
            u, v, vx, vy = st["point_aux"][k][i]
            assert u == synth.FX * p0[0] + synth.CX and v == synth.FY * p0[1] + synth.CY
            if k > 0 and i in st0["points"][k - 1]:
                seen_old += 1
                assert np.array_equal([vx, vy], (p0[:2] - st0["points"][k - 1][i][:2]) / synth.DT_KF)
            else:
                assert vx == 0.0 and vy == 0.0
            want = p0[:2] + (0.004 + 0.02 / synth.IMG_H * (v - synth.IMG_H / 2)) * np.array([vx, vy])
            assert np.array_equal(st["points"][k][i][:2], want) and st["points"][k][i][2] == 1.0
    assert seen_old > 20
    # TR = 0, td_true = 0: nothing moves
    z = replay.simulate_stream_td(3, 5, 0.0, **kw)
    assert all(np.array_equal(z["points"][k][i], st0["points"][k][i]) for k in range(5) for i in st0["points"][k])
