"""GPU parity of the fused sliding-window solve (through the C-ABI batch surface) against the golden trace
and the C oracle on the same seeded windows.  Tolerance: 1e-6 relative on dx and final cost (north_star)."""
import ctypes as C

import numpy as np
import pytest

import orc
import synth
from util import fro, golden_windows, rel, rel_by_family, state_families, sub_window

pytestmark = pytest.mark.gpu
TOL = 1e-6
WORST = {}          # state family -> worst relative error against the oracle over this module (test_zz_report prints it)


def gpu_solve(tcv, wins, iters=8, fixed=True, mfma=True, threads=256, **kw):
    W = [tcv.Window(w, **kw) for w in wins]
    b = tcv.Batch(W)
    b.solve(tcv.default_options(iters, fixed, mfma, threads, True))
    b.synchronize()
    b.download_states()
    return W, b, b.summaries()


def check_states_by_family(sg, st, tol=TOL, tag=None):
    """the gate on the solved states within every parameter family (positions, quaternions, velocities, accelerometer and gyro biases,
    extrinsic translation and rotation, inverse depths): each relative to the oracle's own magnitude in that family"""
    byf = rel_by_family(state_families(sg), state_families(st))
    for name, v in byf.items():
        WORST[name] = max(WORST.get(name, 0.0), v)
        assert v < tol, (tag, name, v)
    return byf


def check_against_oracle(tcv, w, W, b, s, k, iters, fixed, ex_constant=False):
    O = orc.Window(w, ex_constant=ex_constant)
    so = O.solve(iters, fixed)
    assert s.num_iterations == so.num_iterations and s.termination == so.termination
    n = so.num_iterations
    assert [s.dogleg_case[i] for i in range(1, n)] == [so.dogleg_case[i] for i in range(1, n)]
    assert [s.step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
    assert rel([s.cost[i] for i in range(n)], [so.cost[i] for i in range(n)]) < TOL
    assert abs(s.final_cost - so.final_cost) < TOL * so.final_cost
    st, sg = O.states(), W.states()
    for key in ("pose", "sb", "ex", "lam"):
        assert rel(sg[key], st[key]) < TOL, key
    check_states_by_family(sg, st)
    fo = np.array(so.first_delta[:so.n_local]); fg = b.first_step(k)
    assert len(fg) == len(fo) and fro(fg, fo) < TOL
    mg = np.array([s.model_cost_change[i] for i in range(1, n)]); mo = np.array([so.model_cost_change[i] for i in range(1, n)])
    ok = np.array([so.dogleg_case[i] > 0 for i in range(1, n)])
    assert rel(mg[ok], mo[ok]) < 1e-5


def test_golden_window_trace(gpu):
    pre, main, z = golden_windows()
    for w, p in ((pre, "pre_"), (main, "main_")):
        W, b, s = gpu_solve(gpu, [w])
        n = s[0].num_iterations
        assert n == len(z[p + "cost"])
        assert rel([s[0].cost[i] for i in range(n)], z[p + "cost"]) < TOL
        sg = W[0].states()
        assert rel(sg["pose"], z[p + "final_pose"]) < TOL and rel(sg["sb"], z[p + "final_sb"]) < TOL
        assert rel(sg["ex"], z[p + "final_ex"]) < TOL and rel(sg["lam"], z[p + "final_lam"]) < TOL
        check_states_by_family(sg, dict(pose=z[p + "final_pose"], sb=z[p + "final_sb"], ex=z[p + "final_ex"], lam=z[p + "final_lam"]), tag=p)
        assert fro(b.first_step(0), z[p + "first_delta"]) < TOL
        assert [s[0].dogleg_case[i] for i in range(1, n)] == [int(c) for c in z[p + "case"][1:]]


@pytest.mark.parametrize("mfma,threads", [(True, 256), (False, 256), (True, 512)])
def test_cfg2_points_only_vs_oracle(gpu, mfma, threads):
    """BASELINE config 2: 10-kf window, 200 point residual blocks, no lines, no prior (gauge handled by the mu D^2 path)."""
    batch = synth.make_windows(100, 3, with_lines=False)
    wins = [synth.window_at(batch, k) for k in range(3)]
    W, b, s = gpu_solve(gpu, wins, mfma=mfma, threads=threads)
    for k in range(3):
        check_against_oracle(gpu, wins[k], W[k], b, s[k], k, 8, True)


def test_cfg3_points_lines_prior_vs_oracle(gpu):
    """BASELINE config 3: 200 point + 40 line residual blocks + marginalisation prior."""
    pre, main, z = golden_windows()
    batch = synth.make_windows(200, 2)
    wins = [main] + [dict(synth.window_at(batch, k), prior=None) for k in range(2)]
    W, b, s = gpu_solve(gpu, wins)
    for k in range(3):
        check_against_oracle(gpu, wins[k], W[k], b, s[k], k, 8, True)
    assert b.plan_stats()["num_plans"] == 2          # windows with the same graph structure share one plan


def test_run_to_convergence_with_ceres_tolerances(gpu):
    pre, main, z = golden_windows()
    W, b, s = gpu_solve(gpu, [main], iters=50, fixed=False)
    assert s[0].num_iterations == int(z["conv_num_iterations"]) and s[0].termination == int(z["conv_termination"])
    assert abs(s[0].final_cost - float(z["conv_final_cost"])) < TOL * float(z["conv_final_cost"])
    check_against_oracle(gpu, main, W[0], b, s[0], 0, 50, False)


def test_constant_extrinsic(gpu):
    """ESTIMATE_EXTRINSIC == 0: SetParameterBlockConstant(para_Ex_Pose) (estimator.cpp:1694-1698)."""
    batch = synth.make_windows(300, 1)
    w = synth.window_at(batch, 0)
    W, b, s = gpu_solve(gpu, [w], estimate_extrinsic=False)
    assert np.array_equal(W[0].ex, w["ex_pose"])
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 8, True, ex_constant=True)


@pytest.mark.parametrize("frames", [3, 6, 9])
def test_short_and_ragged_windows(gpu, frames):
    batch = synth.make_windows(400, 1)
    w = sub_window(synth.window_at(batch, 0), frames)
    W, b, s = gpu_solve(gpu, [w])
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 8, True)


def test_no_points_imu_and_lines_only(gpu):
    batch = synth.make_windows(500, 1)
    w = dict(synth.window_at(batch, 0))
    pr = w["proj"]
    w["proj"] = {k: (np.asarray(v)[:0] if isinstance(v, np.ndarray) and v.shape[:1] == (200,) else v) for k, v in pr.items()}
    w["lam"] = np.zeros(0)
    W, b, s = gpu_solve(gpu, [w])
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 8, True)


def test_many_landmarks_are_chunked_through_lds(gpu):
    """alternative reading of the config (200 landmarks x 4 observations = 800 blocks): several staging chunks."""
    batch = synth.make_windows(600, 1, n_landmarks=200)
    w = synth.window_at(batch, 0)
    W, b, s = gpu_solve(gpu, [w])
    assert W[0].plan_stats()["n_vis_chunk"] >= 2
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 8, True)


def test_single_problem_ceres_style_entry_point(gpu):
    """tcv_solve(options, problem, summary) updates the caller's parameter blocks in place like ceres::Solve."""
    batch = synth.make_windows(700, 1)
    w = synth.window_at(batch, 0)
    W = gpu.Window(w)
    s = gpu.SolverSummary()
    o = gpu.default_options(8, True)
    gpu.check(gpu.lib().tcv_solve(C.byref(o), W.h, C.byref(s)))
    O = orc.Window(w); so = O.solve(8, True)
    assert abs(s.final_cost - so.final_cost) < TOL * so.final_cost
    assert rel(W.pose, O.states()["pose"]) < TOL and not np.array_equal(W.pose, w["pose"])


def test_max_iterations_zero_and_one(gpu):
    batch = synth.make_windows(800, 1)
    w = synth.window_at(batch, 0)
    W, b, s = gpu_solve(gpu, [w], iters=0)
    assert s[0].num_iterations == 1 and s[0].initial_cost == s[0].final_cost
    assert np.array_equal(W[0].pose, w["pose"])
    W, b, s = gpu_solve(gpu, [w], iters=1)
    check_against_oracle(gpu, w, W[0], b, s[0], 0, 1, True)


def test_chain_layout_matches_dense_layout_and_oracle(gpu):
    """The default chain layout (speed-bias blocks eliminated one by one before the dense pose system, two windows per CU)
    and the dense 171-dim layout solve the same scaled, mu-regularised system: identical dogleg traces, first steps within
    1e-6 of each other (measured 1e-9..1e-8), and both within the north-star tolerance of the C oracle."""
    pre, main, z = golden_windows()
    wins = [pre, main] + [synth.window_at(synth.make_windows(77, 2), k) for k in range(2)]
    out = {}
    try:
        for variant in (0, 1):
            gpu.check(gpu.lib().tcv_set_solver_variant(variant))
            W = [gpu.Window(w) for w in wins]
            b = gpu.Batch(W)
            assert b.plan_stats()["layout"] == ("chain" if variant == 0 else "dense") and b.plan_stats()["lds_bytes"] == 160 * 1024    # a batch smaller than the chip: the whole LDS
            b.solve(gpu.default_options(8, True, True, 256, True)); b.synchronize(); b.download_states()
            s = b.summaries()
            out[variant] = [(s[k].final_cost, [s[k].dogleg_case[i] for i in range(9)], [s[k].step_ok[i] for i in range(9)],
                             W[k].pose.copy(), W[k].sb.copy(), b.first_step(k)) for k in range(len(wins))]
    finally:
        gpu.check(gpu.lib().tcv_set_solver_variant(0))
    for k, w in enumerate(wins):
        O = orc.Window(w); so = O.solve(8, True); st = O.states()
        c, d = out[0][k], out[1][k]
        assert c[1] == d[1] == [so.dogleg_case[i] for i in range(9)] and c[2] == d[2]
        assert rel(c[5], d[5]) < 1e-6
        for v in (c, d):
            assert abs(v[0] - so.final_cost) < 1e-6 * so.final_cost
            assert rel(v[3], st["pose"]) < 1e-6 and rel(v[4], st["sb"]) < 1e-6
            check_states_by_family(dict(pose=v[3], sb=v[4]), dict(pose=st["pose"], sb=st["sb"]), 1e-6, k)


def test_chain_layout_variants_vs_oracle(gpu):
    """graph shapes around the chain layout: a broken IMU chain (sum_dt > 10 drops a factor, estimator.cpp:1726), a prior that
    also holds the neighbouring speed-bias block (still a chain) and one that ties a distant speed-bias block in (dense fallback)."""
    pre, main, z = golden_windows()
    p = main["prior"]
    n = p["n"] + 9
    J0 = np.zeros((n, n)); J0[:p["n"], :p["n"]] = p["J0"]; J0[p["n"]:, p["n"]:] = 30.0 * np.eye(9)
    def with_sb(i):
        return dict(p, n=n, J0=J0, r0=np.concatenate([p["r0"], 0.01 * np.ones(9)]), sizes=list(p["sizes"]) + [9], idx=list(p["idx"]) + [p["n"]],
                    x0=list(p["x0"]) + [np.asarray(main["speedbias"])[i].copy()], blocks=list(p["blocks"]) + [("sb", i)])
    w_broken = dict(pre); im = dict(pre["imu"]); sd = np.array(im["sum_dt"], dtype=float).copy(); sd[4] = 11.0; im["sum_dt"] = sd; w_broken["imu"] = im
    cases = [("broken chain", w_broken, "chain"), ("prior on sb0+sb1", dict(main, prior=with_sb(1)), "chain"), ("prior on sb0+sb5", dict(main, prior=with_sb(5)), "dense")]
    for name, w, layout in cases:
        W = gpu.Window(w)
        b = gpu.Batch([W])
        assert b.plan_stats()["layout"] == layout, name
        b.solve(gpu.default_options(8, True)); b.synchronize(); b.download_states()
        s = b.summaries()[0]
        O = orc.Window(w); so = O.solve(8, True); st = O.states()
        assert abs(s.final_cost - so.final_cost) < 1e-6 * so.final_cost, name
        assert [s.dogleg_case[i] for i in range(9)] == [so.dogleg_case[i] for i in range(9)], name
        assert rel(W.pose, st["pose"]) < 1e-6 and rel(W.sb, st["sb"]) < 1e-6, name
        check_states_by_family(W.states(), st, 1e-6, name)


def test_cxx_examples_run_on_the_device(gpu, tmp_path):
    """examples/estimator_shim.cpp (plain C-ABI) and estimator_shim_classes.cpp (include/tcv_ceres_shim.hpp, the Ceres-shaped classes
    estimator.cpp uses) solve the same toy window: same iterations, cost and inverse depth; the class veneer chains the prior."""
    import os, re, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.LIB_PATH)
    outs = []
    for src in ("estimator_shim.cpp", "estimator_shim_classes.cpp"):
        exe = os.path.join(tmp_path, src[:-4])
        subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", src), "-L" + libdir, "-ltcv_hip",
                               "-Wl,-rpath," + libdir, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    a = re.search(r"solve: (\d+) iterations, cost (\S+) -> (\S+), inverse depth (\S+)", outs[0]).groups()
    b = re.search(r"solve: (\d+) iterations, cost (\S+) -> (\S+), inverse depth (\S+)", outs[1]).groups()
    assert a == b and float(a[2]) < 1e-12 * float(a[1]) and abs(float(a[3]) - 0.1) < 1e-3
    assert "prior: m = 16" in outs[0] and "prior: m = 16" in outs[1] and "first -> para_Pose[0]: yes" in outs[1]
    assert "batched frame: marginalisation status 0, prior m = 16" in outs[0] and "device-resident 1" in outs[0]      # (the no-wait frame loop of INTEGRATION.md 3a)


def test_max_solver_time_stops_the_iteration_loop(gpu):
    """Solver::Options::max_solver_time_in_seconds (estimator.cpp:1892-1897): checked at the start of every iteration; a budget far
    below one iteration leaves only the initial evaluation, a generous one changes nothing."""
    pre, main, z = golden_windows()
    def run(budget, iters=50):
        W = gpu.Window(main); b = gpu.Batch([W])
        o = gpu.default_options(iters, False); o.max_solver_time_in_seconds = budget
        b.solve(o); b.synchronize()
        s = b.summaries()[0]
        return s.num_iterations, s.termination, s.final_cost
    n_free, t_free, c_free = run(0.0)
    n_big, t_big, c_big = run(10.0)
    assert (n_big, t_big, c_big) == (n_free, t_free, c_free) and n_free > 5
    n0, t0, c0 = run(1e-7)
    assert n0 == 1 and t0 == 0                       # iteration 0 only (summary.iterations.size() == 1), NO_CONVERGENCE
    n1, t1, c1 = run(0.0008)                         # ~0.3 ms per iteration for a lone window: a few iterations fit
    assert 1 < n1 < n_free and c0 > c1 > c_free * (1 - 1e-12)


@pytest.mark.parametrize("window", ["prior", "no prior"])
@pytest.mark.parametrize("gone", [(0,), (4,), (7,), (2, 6), (9,)])      # (9,): para_SpeedBias[10] is left without any factor
def test_imu_factor_over_ten_seconds_is_left_out(gpu, gone, window):
    """estimator.cpp:1726: `if (pre_integrations[j]->sum_dt > 10.0) continue;` (a platform that stood still: MARGIN_SECOND_NEW keeps merging
    the IMU buffers of the newest interval) -- the window is then two or three IMU chains (the chain layout's steps cover them,
    tests/test_abi_cpu.py).  The HIP side gets the window WITH the long pre-integration and must drop it itself (tcv_problem_from_window);
    the oracle gets the graph without that factor.  With the prior -- which couples para_SpeedBias[0] to every pose -- this caught the
    chain elimination carrying the first chain's W rows into the second one (round 5)."""
    pre, main0, z = golden_windows()
    main = main0 if window == "prior" else pre
    im = dict(main["imu"])
    sd = np.array(im["sum_dt"], dtype=float).copy(); sd[list(gone)] = 11.0; im["sum_dt"] = sd
    w_hip = dict(main, imu=im)
    keep = ~np.isin(np.arange(len(sd)), gone)
    w_orc = dict(main, imu={k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and np.asarray(v).shape[:1] == keep.shape else v) for k, v in main["imu"].items()})
    W, b, s = gpu_solve(gpu, [w_hip])
    assert gpu.lib().tcv_problem_num_residual_blocks(W[0].h) == len(main["imu"]["sum_dt"]) - len(gone) + len(main["proj"]["frame_i"]) + len(main["line"]["frame"]) + (1 if main.get("prior") is not None else 0)
    assert b.plan_stats()["layout"] == "chain"
    O = orc.Window(w_orc); so = O.solve(8, True)
    n = so.num_iterations
    assert s[0].num_iterations == n and [s[0].step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
    assert [s[0].dogleg_case[i] for i in range(1, n)] == [so.dogleg_case[i] for i in range(1, n)]
    assert abs(s[0].final_cost - so.final_cost) < TOL * so.final_cost
    st, sg = O.states(), W[0].states()
    for key in ("pose", "sb", "ex", "lam"):
        assert rel(sg[key], st[key]) < TOL, key
    check_states_by_family(sg, st, tag=(window, gone))


def test_a_window_beyond_half_a_cu_moves_its_batch_to_one_workgroup_per_cu(gpu):
    """Maximum sizes.  A batch larger than the chip runs two workgroups per CU on 80 KiB of LDS each, which holds windows of up to ~280
    landmarks; ONE larger window (here 600 landmarks x 4 observations = 2400 point factors, twelve staging chunks) used to fail the whole
    tcv_batch_create with TCV_ERR_TOO_LARGE -- the batch now takes one workgroup per CU with all 160 KiB (up to 1024 landmarks).  Both the
    large window and its small neighbours must come out as the oracle solves them."""
    small = synth.make_windows(5200, 300)
    wins = [synth.window_at(small, k) for k in range(300)]
    wins[137] = synth.window_at(synth.make_windows(5600, 1, n_landmarks=600), 0)
    W = [gpu.Window(w) for w in wins]
    b = gpu.Batch(W)
    num, pbytes, grid, lds = b.plan_stats()["num_plans"], b.plan_stats()["plan_bytes"], b.plan_stats()["grid"], b.plan_stats()["lds_bytes"]
    assert lds == 160 * 1024 and grid <= 256 and num == 2
    b.solve(gpu.default_options(8, True, True, 256, True)); b.synchronize(); b.download_states()
    s = b.summaries()
    for k in (137, 0, 299):
        check_against_oracle(gpu, wins[k], W[k], b, s[k], k, 8, True)
    # the limit itself: 1024 landmarks pack, 1025 are refused with a clear error
    big = gpu.Window(synth.window_at(synth.make_windows(5700, 1, n_landmarks=1024), 0))
    b1 = gpu.Batch([big]); b1.solve(gpu.default_options(2, True)); b1.synchronize()
    assert np.isfinite(b1.summaries()[0].final_cost)
    with pytest.raises(gpu.TcvError):
        gpu.Batch([gpu.Window(synth.window_at(synth.make_windows(5800, 1, n_landmarks=1025), 0))])


@pytest.mark.parametrize("seed", [156, 240, 58, 258])
@pytest.mark.parametrize("layout", ["chain", "dense"])
def test_rank_deficient_windows_keep_the_oracles_accuracy(gpu, seed, layout):
    """Windows whose camera system is rank deficient beyond the gauge -- two frames without a prior (156, 240), a pose held by one observation
    and no IMU factor (58, 258: the pre-integrations over 10 s at the end of the window are left out) -- are held by the trust region's mu D^2
    alone (condition ~1e9).  The tiled Cholesky's panel solve used to multiply by the explicit inverse of the diagonal tile on the matrix
    cores, which is not backward stable: first steps off by 1e-3 .. 1e-4 on these windows while the oracle is within 1e-7 of the 50-digit
    solution (tests/dev/fuzz_solve.py found them, tests/dev/fuzz_one.py has the 50-digit comparison).  With one refinement step in the panel
    the device is as close as the oracle; the gate is the north_star's 1e-6 on the first step and the final cost."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev"))
    import fuzz_solve as fz
    rng = np.random.Generator(np.random.PCG64(seed))
    w_hip, w_orc, exc, note = fz.make_case(rng, seed)
    O = orc.Window(w_orc, ex_constant=exc); so = O.solve(8, True)
    Ws, b, s = fz.gpu_run(w_hip, exc, copies=1, dense=(layout == "dense"))
    assert b.plan_stats()["layout"] == layout
    fo = np.array(so.first_delta[:so.n_local]); fg = b.first_step(0)
    assert len(fg) == len(fo) and fro(fg, fo) < TOL, note
    n = so.num_iterations
    if so.final_cost < 1e-12:      # (seed 156 ends on a zero-residual fit, cost 1e-23: the acceptance tests of the last iterations compare rounding noise)
        assert s[0].final_cost < 1e-12
        return
    assert s[0].num_iterations == n and [s[0].step_ok[i] for i in range(1, n)] == [so.step_ok[i] for i in range(1, n)]
    # eight iterations from a cost of 1e7 on a condition of 1e9: every rounding order ends on digits of its own -- seed 258: 255.19562 (chain),
    # 255.19508 (dense), 255.19312 (dense, substitution), 255.19689 (oracle); the first step above is the well-posed gate
    assert abs(s[0].final_cost - so.final_cost) < 2e-5 * max(so.final_cost, 1e-12), note


def test_zz_report():
    for k, v in WORST.items():
        print("worst solved-state error against the oracle, %-8s %.3e" % (k, v))
