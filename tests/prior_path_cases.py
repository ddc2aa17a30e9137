"""Test helper for the residency paths of the marginalisation prior in tcv::solve_kernel (tests/test_prior_paths_cpu.py,
tests/test_gpu_prior_paths.py).  No GPU import: everything here runs on the packer's host side and the oracles.

The prior enters the kernel by five code paths, chosen at run time from the LDS budget of the window's plan:

  part A (linearize: r = r0 + J0 dx, J0' r)   in_lds   J0 staged once
                                              staged   chain layout only: J0 through the pool in two column pieces [0, ns), [ns, n)
                                              global   straight from global memory
  setup  (Hp = J0' J0, once per solve)        lds      2 x 2 blocks out of LDS, column stride nr | 1 where that fits, else nr
                                              global   entry by entry from global memory

`plan_header` reads the plan the packer builds for a window (tcv_problem_plan_ints: the half-CU budget, the policy of batches larger than
the chip) and `prior_paths` evaluates the kernel's own predicates on it -- a mirror of tcv_solve.hip (part A: the block that begins
`if (P.prior_n > 0 && ABL(C, AB_PRIOR_A))`, its `if (staged)` branch; setup: `if (P.prior_n > 0 && ABL(C, AB_SETUP))`), named in a comment
at each of the three sites.  The case builders shape priors that land on a chosen path; `chain_cases` / `dense_cases` are the named cases
both test files run, with the path each is pinned to."""
import ctypes as C
import types

import numpy as np

import np_oracle as NO
import synth
from util import golden_windows, sub_window

# PlanHdr of csrc/tcv_packed.h, field by field
HDR_FIELDS = ("nblk nland nc nx npp nt ntp n_imu n_proj n_line prior_n prior_nblk prior_xsize hcl_total n_imu_chunk n_vis_chunk lds_area flags "
              "td_cam camw o_blk o_imu o_proj o_line o_prior o_pcol o_pdest o_lm o_lmslot o_lmslotptr o_vchunk o_vdest o_vunit o_vitem n_vdest "
              "n_vunit n_vitem o_sdest o_sunit o_sitem n_sdest n_sunit n_sitem o_ichunk o_idest o_iunit o_iitem n_idest n_iunit n_iitem chain n_e "
              "nt_c c_stage_cap c_area_cap c_pool c_spill o_chain n_frames o_frames plan_ints").split()
_LOCAL = {"pose": 6, "sb": 9, "ex": 6, "td": 1}
_GLOBAL = {"pose": 7, "sb": 9, "ex": 7, "td": 1}


def plan_ints(tcv, W):
    L = tcv.lib()
    L.tcv_problem_plan_ints.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    n = C.c_int()
    tcv.check(L.tcv_problem_plan_ints(W.h, None, 0, C.byref(n)))
    out = np.zeros(n.value, np.int32)
    tcv.check(L.tcv_problem_plan_ints(W.h, out.ctypes.data_as(C.POINTER(C.c_int)), n.value, C.byref(n)))
    return out


def plan_header(tcv, W):
    """the PlanHdr of the plan tcv_problem_plan_ints builds for W, as a namespace.  Guards against a header whose layout has moved on:
    the fields plan_stats() reports by name have to agree, and plan_ints -- the last field -- has to be the length of the pool behind it."""
    v = plan_ints(tcv, W)
    nh = len(HDR_FIELDS)
    assert len(v) >= nh, (len(v), nh)
    h = types.SimpleNamespace(**{k: int(x) for k, x in zip(HDR_FIELDS, v[:nh])})
    st = W.plan_stats()
    assert (h.nc, h.nx, h.nland, h.n_vis_chunk) == (st["nc"], st["nx"], st["nland"], st["n_vis_chunk"]), (h, st)
    assert h.chain in (0, 1) and (h.nt_c if h.chain else h.nt) == st["nt"], (h, st)
    assert h.plan_ints == len(v) - nh == st["plan_ints"], (h.plan_ints, len(v) - nh, st["plan_ints"])
    return h


def prior_zero_rows(J0, r0):
    """prior_zero_rows of csrc/tcv_packed.h: the leading rows of J0 | r0 that are exact zeros; one row is always kept"""
    J0 = np.asarray(J0, dtype=float); r0 = np.asarray(r0, dtype=float)
    n = J0.shape[0]
    k0 = 0
    while k0 < n and r0[k0] == 0.0 and not J0[k0].any():
        k0 += 1
    return k0 if k0 < n else (n - 1 if n > 0 else 0)


def _cdiv(a, b):      # C's integer division (towards zero)
    return int(a / b) if (a < 0) != (b < 0) else a // b


def prior_paths(hdr, k0):
    """The kernel's predicates on a plan header: dict(part_a in_lds | staged | global, nb, ns (the two pieces [0, ns), [ns, n) of the
    staged path; nb = n, ns = 0 where J0 is not split), setup lds | global, ldj (column stride of J0 in the setup's LDS copy; None on the
    global path), n, nr)."""
    n, chain = hdr.prior_n, bool(hdr.chain)
    nr = n - k0
    ntd = hdr.nt_c if chain else hdr.nt
    ntiles, pp_tiles = ntd * (ntd + 1) // 2, hdr.ntp * (hdr.ntp + 1) // 2
    # part A
    stage_cap = hdr.c_stage_cap if chain else (ntiles - pp_tiles) << 8
    in_lds = ((nr * n + 1) & ~1) + 2 * n <= stage_cap
    pcap = _cdiv(hdr.c_pool - 2 * n - 2, nr) - 1 if chain else 0
    staged = chain and not in_lds and n - pcap <= pcap
    nb, ns = n, 0
    if staged:
        nb = min(n, pcap + 1)
        if (nr & 1) and ((n - nb) & 1):
            nb -= 1
        ns = n - nb
    # setup
    lds_cap = (ntiles << 8) + (hdr.c_pool if chain else 0)
    setup_lds = nr * n <= lds_cap
    ldj = ((nr | 1) if (nr | 1) * n <= lds_cap else nr) if setup_lds else None
    return dict(part_a="staged" if staged else "in_lds" if in_lds else "global", nb=nb, ns=ns, setup="lds" if setup_lds else "global", ldj=ldj,
                n=n, nr=nr, layout="chain" if chain else "dense", stage_cap=stage_cap, pcap=pcap, lds_cap=lds_cap)


# ---- case builders ---------------------------------------------------------------------------------------------------------------
def with_stored_rows(w, nr):
    """the window with the last nr - (n - k0) leading zero rows of its prior replaced by a weak diagonal (1e-2), so that the prior has nr
    stored rows (tests/test_gpu_solve_paths.py::test_prior_without_zero_rows does it to all of them)"""
    p = w["prior"]
    J0 = np.array(p["J0"], dtype=float)
    k0 = prior_zero_rows(J0, p["r0"])
    n = int(p["n"])
    more = nr - (n - k0)
    assert 0 <= more <= k0, (nr, n, k0)
    for i in range(k0 - more, k0):
        J0[i, i] = 1e-2
    assert prior_zero_rows(J0, p["r0"]) == n - nr
    return dict(w, prior=dict(p, J0=J0))


def with_block_at(w, block, pos):
    """the window with `block` of its prior moved to position `pos` of the prior's block order (the columns of J0 move with it): the same
    prior in another column order"""
    p = w["prior"]
    blocks = [tuple(b) for b in p["blocks"]]
    order = [k for k in range(len(blocks)) if blocks[k] != tuple(block)]
    order.insert(pos, blocks.index(tuple(block)))
    J_old = np.asarray(p["J0"], dtype=float)
    J0 = np.zeros_like(J_old)
    idx, o = [], 0
    for k in order:
        ls = 6 if p["sizes"][k] == 7 else p["sizes"][k]
        J0[:, o:o + ls] = J_old[:, p["idx"][k]:p["idx"][k] + ls]
        idx.append(o); o += ls
    assert o == p["n"]
    return dict(w, prior=dict(p, blocks=[blocks[k] for k in order], sizes=[p["sizes"][k] for k in order], x0=[p["x0"][k] for k in order], idx=idx, J0=J0))


def window_blocks(w, names=("pose", "sb", "ex")):
    """every pose, every speed-bias block and the extrinsic of a window (then para_Td where asked for), as a prior's block list"""
    F = len(w["pose"])
    out = []
    for nm in names:
        out += [(nm, i) for i in range(F)] if nm in ("pose", "sb") else [(nm, 0)]
    return out


def _state(w, nm, i):
    if nm == "pose":
        return np.array(w["pose"][i], dtype=float)
    if nm == "sb":
        return np.array(w["speedbias"][i], dtype=float)
    if nm == "ex":
        return np.array(w["ex_pose"], dtype=float)
    return np.array([float(w["td"])])


def hand_prior(w, blocks, nr, seed, step=1e-2, sigma_j=3.0, sigma_r=0.05):
    """A prior over `blocks` of the window, made by hand: x0 = the window's states moved by a seeded tangent step ~ N(0, step) (dx != 0 at
    the start), J0 ~ N(0, sigma_j) in its last nr rows and r0 ~ N(0, sigma_r) there, exact zeros above."""
    rng = np.random.default_rng(seed)
    sizes = [_GLOBAL[nm] for nm, i in blocks]
    local = [_LOCAL[nm] for nm, i in blocks]
    idx = [int(v) for v in np.concatenate([[0], np.cumsum(local)[:-1]])]
    n = int(sum(local))
    assert 1 <= nr <= n
    x0 = []
    for (nm, i), ls in zip(blocks, local):
        x, d = _state(w, nm, i), step * rng.normal(size=ls)
        x0.append(NO.pose_plus(x, d) if nm in ("pose", "ex") else x + d)
    J0 = np.zeros((n, n)); r0 = np.zeros(n)
    J0[n - nr:] = sigma_j * rng.normal(size=(nr, n))
    r0[n - nr:] = sigma_r * rng.normal(size=nr)
    return dict(m=0, n=n, sizes=sizes, idx=idx, blocks=list(blocks), x0=x0, J0=J0, r0=r0)


def fillers(k, seed=5300):
    """k cheap windows that take the chain layout: 3-frame cuts of synthetic windows, no prior"""
    batch = synth.make_windows(seed, k)
    return [sub_window(synth.window_at(batch, i), 3) for i in range(k)]


def with_landmarks(w, n_land, seed):
    """the window with the point factors and landmarks of a synthetic window of n_land landmarks (tests/test_pack_cpu.py does the same)"""
    big = synth.window_at(synth.make_windows(seed, 1, n_landmarks=n_land), 0)
    return dict(w, proj=big["proj"], lam=big["lam"])


# ---- the named cases -------------------------------------------------------------------------------------------------------------
# name -> what the plan of tcv_problem_plan_ints (chain layout, half-CU budget) must give: part_a, nb, ns, setup
CHAIN_EXPECTED = {
    "nr41_control": ("in_lds", 75, 0, "lds"),
    "nr54_last_in_lds": ("in_lds", 75, 0, "lds"),
    "nr55_one_piece": ("staged", 75, 0, "lds"),
    "nr66_ns1": ("staged", 74, 1, "lds"),
    "nr67_ns2": ("staged", 73, 2, "lds"),
    "nr73_ns8": ("staged", 67, 8, "lds"),
    "nr75_ns10": ("staged", 65, 10, "lds"),
    "nr75_L90_aligned": ("staged", 63, 12, "lds"),
    "nr75_ex_constant": ("staged", 65, 10, "lds"),
    "td_full_rank": ("staged", 64, 12, "lds"),      # n = 76: the golden prior's blocks and para_Td
}
# name -> (part_a, setup, ldj); the dense layout under both tcv_set_solver_variant values
DENSE_EXPECTED = {
    "f3_nr33": ("in_lds", "lds", 33),
    "f3_nr34": ("global", "lds", 35),
    "f3_nr50": ("global", "lds", 50),
    "f3_nr51": ("global", "global", None),
    "f4_nr66": ("global", "global", None),
}
_CACHE = {}


def chain_cases():
    """name -> (window, ex_constant).  The golden main window's structure (50 landmarks) with its own prior padded to nr stored rows,
    unless the name says otherwise."""
    if "chain" in _CACHE:
        return dict(_CACHE["chain"])
    pre, main, z = golden_windows()
    out = {}
    for name in CHAIN_EXPECTED:
        if name.startswith("nr") and "_L90" not in name and "_ex" not in name:
            out[name] = (with_stored_rows(main, int(name[2:4])), False)
    # (seed 1990, not the 990 of tests/test_pack_cpu.py: on that window eight iterations end in a slow valley -- the cost still falls by 4 % in
    # the last one -- and the two oracles themselves end 2.2e-7 apart in the inverse depths, against 3e-9 .. 4e-8 on seeds 1990 .. 4990 and
    # the golden window; the device, whose usual distance from the C oracle is ten times the oracles' own, ends 2.7e-6 away there on BOTH
    # residency policies with a first step within 7.7e-9.  The first step is sound on both windows -- C oracle 2.5e-9 / 2.2e-9, np_oracle
    # 1.8e-9 / 1.6e-9 from the 50-digit solution (make_golden_pins.mp_first_step) on 990 / 1990 --: what 990 amplifies is the trajectory of
    # eight iterations.  On 1990 the oracles end 6.6e-9 apart.)
    out["nr75_L90_aligned"] = (with_stored_rows(with_landmarks(main, 90, 1990), 75), False)
    # the extrinsic held constant, its block moved behind para_Pose[0]: columns 6 .. 11 have pcol < 0, four in the first piece, two in the second
    out["nr75_ex_constant"] = (with_stored_rows(with_block_at(main, ("ex", 0), 1), 75), True)
    wt = synth.with_time_offset(synth.window_at(synth.make_windows(918, 1), 0), 918)
    blocks = [tuple(b) for b in main["prior"]["blocks"]] + [("td", 0)]
    out["td_full_rank"] = (dict(wt, prior=hand_prior(wt, blocks, 76, seed=918)), False)
    _CACHE["chain"] = out
    return dict(out)


def dense_cases():
    """name -> (window, ex_constant): 3- and 4-frame windows with a hand-made prior over every pose, every speed-bias block and the
    extrinsic (no speed-bias chain is left, so both solver variants pack them dense)"""
    if "dense" in _CACHE:
        return dict(_CACHE["dense"])
    out = {}
    for name in DENSE_EXPECTED:
        frames, nr = int(name[1]), int(name[-2:])
        w = sub_window(synth.window_at(synth.make_windows(5400 + frames, 1), 0), frames)
        out[name] = (dict(w, prior=hand_prior(w, window_blocks(w), nr, seed=100 * frames + nr)), False)
    _CACHE["dense"] = out
    return dict(out)


def oracle_first(w, ex_constant=False):
    """(initial cost, first step) of the oracle on a window: the C oracle, np_oracle for an ESTIMATE_TD window (the C oracle has no
    ProjectionTdFactor)"""
    if w.get("td") is not None:
        x, so = NO.solve(NO.Problem(w, ex_constant=ex_constant), 1, True)
        return so["initial_cost"], np.asarray(so["iterations"][1]["delta"])
    import orc
    so = orc.Window(w, ex_constant=ex_constant).solve(1, True)
    return so.initial_cost, np.array(so.first_delta[:so.n_local])


def prior_changes(w, ns):
    """name -> the window with one change to its prior: the columns of the first piece zeroed (where there is one), those of the second
    piece, the last stored row"""
    p = w["prior"]
    out = {}
    for name, rows, cols in (("columns [0, ns)", slice(None), slice(0, ns)), ("columns [ns, n)", slice(None), slice(ns, None)),
                             ("last stored row", slice(-1, None), slice(None))):
        if name == "columns [0, ns)" and ns == 0:
            continue
        J0 = np.array(p["J0"], dtype=float)
        J0[rows, cols] = 0.0
        out[name] = dict(w, prior=dict(p, J0=J0))
    return out


def case_paths(tcv, w, ex_constant=False):
    W = tcv.Window(w, estimate_extrinsic=not ex_constant)
    p = w["prior"]
    return prior_paths(plan_header(tcv, W), prior_zero_rows(p["J0"], p["r0"]))
