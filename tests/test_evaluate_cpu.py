"""Problem::Evaluate surface (include/tcv.h: tcv_batch_evaluate, tcv_problem_evaluate, ...) without a device: defaults, argument
validation and the no-device error of every compute entry point.  (What needs a resident batch -- window indices, capacities,
`at = solution` before a solve, outputs that were not asked for -- is validated in tests/test_gpu_evaluate.py: a batch cannot be
created without a device.)"""
import ctypes as C

import numpy as np
import pytest

import synth


@pytest.fixture(scope="module")
def tcv(built):
    import tcv
    return tcv


def test_evaluate_options_default(tcv):
    o = tcv.EvaluateOptions(at=7, apply_loss_function=0, want_residuals=3, want_gradient=3, want_block_costs=3)
    tcv.lib().tcv_evaluate_options_default(C.byref(o))
    assert (o.at, o.apply_loss_function, o.want_residuals, o.want_gradient, o.want_block_costs) == (tcv.EVALUATE_AT_INITIAL, 1, 0, 0, 0)
    tcv.lib().tcv_evaluate_options_default(None)          # NULL: no crash
    assert C.sizeof(tcv.EvaluateOptions) == 20


def test_evaluate_null_arguments_are_invalid(tcv):
    L = tcv.lib()
    o = tcv.evaluate_options(residuals=True, gradient=True, block_costs=True)
    d = np.zeros(8)
    assert L.tcv_batch_evaluate(None, C.byref(o), None) == tcv.TCV_ERR_INVALID and b"null" in L.tcv_last_error()
    assert L.tcv_batch_evaluation_dims(None, 0, None, None, None) == tcv.TCV_ERR_INVALID
    assert L.tcv_batch_get_evaluation(None, 0, tcv.dptr(d), None, None, None, 0, None, 0, None, 0) == tcv.TCV_ERR_INVALID
    assert L.tcv_batch_get_evaluation_costs(None, tcv.dptr(d), None, None, 1) == tcv.TCV_ERR_INVALID
    assert L.tcv_problem_evaluate(None, C.byref(o), tcv.dptr(d), None, None, None) == tcv.TCV_ERR_INVALID
    W = tcv.Window(synth.window_at(synth.make_windows(5, 1), 0))
    assert L.tcv_problem_evaluate(W.h, None, tcv.dptr(d), None, None, None) == tcv.TCV_ERR_INVALID
    assert L.tcv_problem_num_effective_parameters(None) == 0


def test_num_effective_parameters_counts_the_tangent_sizes_of_free_blocks(tcv):
    w = synth.window_at(synth.make_windows(5, 1), 0)
    F, L = w["pose"].shape[0], w["lam"].shape[0]
    assert tcv.lib().tcv_problem_num_effective_parameters(tcv.Window(w).h) == 15 * F + 6 + L
    assert tcv.lib().tcv_problem_num_effective_parameters(tcv.Window(w, estimate_extrinsic=False).h) == 15 * F + L


def test_problem_evaluate_without_a_device_is_an_error_not_a_crash(tcv):
    w = synth.window_at(synth.make_windows(5, 1), 0)
    W = tcv.Window(w)
    if tcv.lib().tcv_device_count() > 0:          # run where a device is visible: the call simply works
        assert np.isfinite(W.evaluate()["cost"])
        return
    before = W.states()
    with pytest.raises(tcv.TcvError) as e:
        W.evaluate()
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE
    o = tcv.evaluate_options()
    cost = C.c_double(-1.0)
    assert tcv.lib().tcv_problem_evaluate(W.h, C.byref(o), C.byref(cost), None, None, None) == tcv.TCV_ERR_NO_DEVICE and cost.value == -1.0
    for k, v in before.items():
        assert np.array_equal(v, W.states()[k])
    with pytest.raises(tcv.TcvError) as e:          # the batch entry points need a batch, and a batch needs a device
        tcv.Batch([W])
    assert e.value.status == tcv.TCV_ERR_NO_DEVICE
