"""CPU tests of the marginalisation packer (tc-viml_amd/csrc/tcv_marg_host.cpp pack_marg): the plans tcv_problem_marg_plan dumps, without a
device, against tests/golden/marg_plans.npz -- recorded from the packer before it was cut into phases (tests/golden/
make_golden_marg_plans.py) -- int for int, and the host's copy of the kernel's LDS carve against the recorded headers."""
import numpy as np
import pytest

import marg_plan_cases as mpc
from util import load


@pytest.fixture(scope="module")
def tcv(built):
    import tcv
    return tcv


@pytest.fixture(scope="module")
def golden():
    return load("marg_plans.npz")


def _headers(tcv, golden):
    """(case, mode, MargHdr, ints) of every recorded plan that is neither refused nor empty"""
    out = []
    for key in golden.files:
        if key.endswith("__ints") and golden[key].size:
            name, mode, _ = key.split("__")
            out.append((name, mode, mpc.header(tcv, golden[key]), golden[key]))
    return out


def test_plans_are_the_recorded_ones_int_for_int(tcv, golden):
    """every case, stand-alone and next to its solve problem: the ints in full, the length of the double pool and the SHA-256 of each of
    its sections; for a refused problem the return code and the error text"""
    seen = set()
    for name, (build, env) in mpc.cases(tcv).items():
        for mode in ("alone", "solve"):
            rec = mpc.record(tcv, build, env, mode == "solve")
            for k, v in rec.items():
                key = "%s__%s__%s" % (name, mode, k)
                assert key in golden.files, key
                want = golden[key]
                assert v.shape == want.shape and np.array_equal(v, want), (key, v.tobytes()[:200] if k == "err" else (v != want).nonzero())
                seen.add(key)
    assert seen == set(golden.files), set(golden.files) - seen


def test_recorded_cases_cover_every_path_of_the_packer(tcv, golden):
    """the comparison above cannot pass on an easy subset: both modes, at least two chunks, ProjectionTdFactors, both kinds of factor
    sets, shared and own copies of the prior and of the IMU constants, the solve's sqrt_info, C in region P and behind the staging
    records, the empty result and the four refusals"""
    H = [h for _, _, h, _ in _headers(tcv, golden)]
    assert {h.block_mode for h in H} == {0, 1}
    assert any(h.n_pchunk >= 2 for h in H)
    assert any(h.td_blk >= 0 and h.block_mode == 0 for h in H) and any(h.td_blk >= 0 and h.block_mode == 1 for h in H)
    assert {h.proj_disjoint for h in H} == {0, 1}
    assert any(h.prior_abs >= 0 for h in H) and any(h.prior_abs < 0 and h.prior_n > 0 for h in H)
    assert any(h.imu_abs >= 0 for h in H) and any(h.imu_abs < 0 and h.n_imu > 0 for h in H)
    assert any(h.sqrt_src >= 0 for h in H)
    lay = [(h, tcv.marg_lds_layout(h.pos, h.m, h.n, h.nx, h.cb_off, h.cb_stride)) for h in H if h.cb_off >= 0]
    assert any(h.cb_off < L["p"] for h, L in lay) and any(h.cb_off >= L["p"] + 64 * 43 for h, L in lay)
    assert any(h.block_mode == 1 and h.n_pchunk == 0 for h in H)      # (block mode on the factor-by-factor path)
    for mode in ("alone", "solve"):
        assert golden["keeps_nothing__%s__ints" % mode].size == 0 and golden["keeps_nothing__%s__dlen" % mode][0] == 0
        assert golden["keeps_nothing__%s__rc" % mode][0] == 0
        rcs = {c: int(golden["%s__%s__rc" % (c, mode)][0]) for c in ("err_drop_not_in_problem", "err_line_factors", "err_m0", "err_mixed_td")}
        assert rcs == {"err_drop_not_in_problem": tcv.TCV_ERR_INVALID, "err_line_factors": tcv.TCV_ERR_UNSUPPORTED, "err_m0": tcv.TCV_ERR_INVALID,
                       "err_mixed_td": tcv.TCV_ERR_UNSUPPORTED}
    # each switch changes the plan of the case it is set on
    for sw, base in (("switch_proj_serial", "old_prior"), ("switch_own_imu", "old_prior"), ("switch_own_prior", "old_prior"), ("switch_block_serial", "block")):
        a, b = golden[sw + "__solve__ints"], golden[base + "__solve__ints"]
        assert a.shape != b.shape or not np.array_equal(a, b), sw


def test_host_lds_carve_agrees_with_the_recorded_headers(tcv, golden):
    """marg_lds_layout (the host's copy of marg_kernel's LDS carve) against what the packer recorded: C lies at one of the two offsets the
    carve allows, in region P whenever it has room there; the window fits a CU's LDS; and the mode is the carve's answer for the one-piece
    numbering (every dropped dim through the eigen step): one piece exactly when that fits"""
    checked = 0
    for name, mode, h, ints in _headers(tcv, golden):
        L = tcv.marg_lds_layout(h.pos, h.m, h.n, h.nx, h.cb_off, h.cb_stride)
        assert L["total"] <= 20480 and L["p"] % 2 == 0, (name, mode, L)
        if h.cb_off >= 0:
            assert h.cb_stride == (h.pos + 15) // 16 * 16
            assert h.cb_off == (L["cb_off_p"] if L["cb_off_p"] >= 0 else L["cb_off_r2"]), (name, mode, h.cb_off, L)
            assert L["cb_in_r2"] == (0 if L["cb_off_p"] >= 0 else 16 * h.cb_stride + 32)
        else:
            assert L["cb_in_r2"] == 0
        nh = len(bytes(h)) // 4
        mloc = ints[nh + h.o_blk:nh + h.o_blk + 5 * h.nblk].reshape(h.nblk, 5)[:, 2]
        n_pivot = int((mloc <= -2).sum())
        assert (n_pivot > 0) == (h.block_mode == 1)
        one = tcv.marg_lds_layout(h.pos + n_pivot, h.m + n_pivot, h.n, h.nx)
        assert one["fits"] == (h.block_mode == 0), (name, mode, one)
        checked += 1
    assert checked == 28      # 14 cases that pack, twice
