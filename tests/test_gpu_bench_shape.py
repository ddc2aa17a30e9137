"""The BENCHMARKED launch shape against the C oracle (round-3 review, item 1a): what `bench.py` times is
`solve_kernel<256,true,true,false,false>` at two workgroups per CU (80 KiB of LDS each, three visual chunks) and `marg_kernel<256>`
on GPU-made n = 75 priors -- every other oracle comparison of the suite uses a handful of windows, which run in the cooperative
instance or with the whole LDS.  Here 512 benchmark windows (> 256 CUs => one workgroup per window, two per CU) go through
solve -> gauge fix -> marginalisation exactly as in `bench.py`, and every window is compared with oracle/tcv_oracle.c:
identical dogleg / accept traces, final cost, states, A', b' (reference: estimator.cpp:1888-1905, marginalization_factor.cpp:174-299)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from util import fro, rel, rel_by_family, state_families

pytestmark = pytest.mark.gpu

B = 512


def test_benchmark_launch_shape_vs_oracle(gpu):
    import bench
    import np_oracle as NO
    import orc

    batch, wins, keep = bench.build_batches(gpu, synth, 310000, B)
    Wm = keep[0]
    ps = batch.plan_stats()
    assert ps["layout"] == "chain" and ps["lds_bytes"] == 80 * 1024, ps           # the half-CU shape, not the whole-LDS one
    batch.solve(gpu.default_options(bench.SOLVER_ITERATIONS, True)); batch.gauge_fix(); batch.marginalize()
    batch.synchronize(); batch.download_states(); batch.download_priors()
    assert batch.cooperative()["last_solve_workgroups"] == 1                    # not the cooperative instance
    assert ps["grid"] == B, ps                                                  # one workgroup per window, two resident per CU
    s = batch.summaries()
    st = batch.marg_status()
    assert list(st) == [0] * B, {int(k): int((st == k).sum()) for k in np.unique(st)}      # no window on the eigen safety net
    worst = dict(cost=0.0, pose=0.0, sb=0.0, lam=0.0, A=0.0, b=0.0)
    worst_family = {}          # the same states within every parameter family, each relative to the oracle's own magnitude there
    diff_trace = []
    for k in range(B):
        O = orc.Window(wins[k]); so = O.solve(bench.SOLVER_ITERATIONS, True); x = O.states()
        n = so.num_iterations
        assert s[k].num_iterations == n == bench.SOLVER_ITERATIONS + 1
        if [s[k].dogleg_case[i] for i in range(n)] != [so.dogleg_case[i] for i in range(n)] or [s[k].step_ok[i] for i in range(n)] != [so.step_ok[i] for i in range(n)]:
            diff_trace.append(k)
            continue
        R0 = NO.q2R(np.asarray(wins[k]["pose"])[0, 3:]); P0 = np.asarray(wins[k]["pose"])[0, :3]
        Rs, Ps, Vs, po = orc.gauge_fix(R0, P0, x["pose"], x["sb"])
        sb = x["sb"].copy(); sb[:, :3] = Vs
        worst["cost"] = max(worst["cost"], abs(s[k].final_cost - so.final_cost) / so.final_cost)
        worst["pose"] = max(worst["pose"], rel(Wm[k].pose, po)); worst["sb"] = max(worst["sb"], rel(Wm[k].sb, sb))
        worst["lam"] = max(worst["lam"], rel(Wm[k].lam, x["lam"]))
        for name, v in rel_by_family(state_families(dict(pose=Wm[k].pose, sb=Wm[k].sb, ex=Wm[k].ex, lam=Wm[k].lam)),
                                     state_families(dict(pose=po, sb=sb, ex=x["ex"], lam=x["lam"]))).items():
            worst_family[name] = max(worst_family.get(name, 0.0), v)
        w2 = dict(wins[k], pose=po, speedbias=sb, ex_pose=x["ex"], lam=x["lam"])
        pref, dbg = orc.Window(w2).marginalize_old()
        P = batch.prior(k)
        m, n_, nb, xs = P.dims()
        assert (m, n_) == (pref["m"], pref["n"]), k
        As, bs = P.schur()
        worst["A"] = max(worst["A"], fro(As, dbg["A_schur"])); worst["b"] = max(worst["b"], fro(bs, dbg["b_schur"]))
    print("benchmark shape, %d windows vs the C oracle: %d traces differ; worst relative errors %s" % (B, len(diff_trace), {k: float("%.3g" % v) for k, v in worst.items()}))
    assert not diff_trace, diff_trace
    # gates: one order above profiles/r03_parity_sweep.txt (4096 windows: cost 4.4e-8, poses 1.3e-8, speed-biases 3.3e-8,
    # inverse depths 2.7e-7, A' 3.6e-7, b' 2.8e-7); north_star: 1e-6 on the final cost and the step
    assert worst["cost"] < 5e-7 and worst["pose"] < 2e-7 and worst["sb"] < 4e-7 and worst["lam"] < 3e-6, worst
    assert worst["A"] < 4e-6 and worst["b"] < 3e-6, worst
    print("benchmark shape, worst relative error of the states per family: %s" % {k: float("%.3g" % v) for k, v in worst_family.items()})
    assert all(v < 1e-6 for v in worst_family.values()), worst_family


def test_plain_line_and_dumped_outputs_of_the_timed_path(gpu, tmp_path):
    """`bench.py --dump-outputs DIR`: float64 .npy files within 64 MB, the same bits from two runs with the same arguments, and the numbers
    of the timed path itself -- the same windows solved, gauge-fixed and marginalised here in-process.  The plain line carries the headline
    keys, `steps` timed steps and none of the --full figures."""
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps, lines = [], []
    for r in range(2):
        d = tmp_path / ("dump%d" % r)
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--windows", str(B),
                            "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        dumps.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - B) < 1e-6 * B
    assert not {"kernel_ms", "roofline", "roofline_fp64", "cpu_baseline", "batch_sweep", "stream_solves_per_s", "replay_windows_per_s"} & set(line)
    a, b = dumps
    assert sorted(a) == sorted(b) and {"pose", "speedbias", "inv_depth", "final_cost", "prior_J0", "prior_r0", "prior_A", "prior_b"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float64 and a[k].tobytes() == b[k].tobytes(), k
    ws = a["window"].astype(int); ps = a["prior_window"].astype(int)
    assert list(ws) == list(range(B)) and len(ps) == bench.DUMP_PRIOR_WINDOWS and len(set(ps)) == len(ps)

    batch, wins, keep = bench.build_batches(gpu, synth, bench.shard_ids(0, B), B)
    bench.fuse(batch)
    batch.solve(gpu.default_options(bench.SOLVER_ITERATIONS, True, True, 256)); batch.gauge_fix(); batch.marginalize()
    Wm = keep[0]
    # the same dump in-process: the same numbers, and the caller's blocks (shared with the marginalisation windows) hold their INITIAL states
    # afterwards -- the --full figures build new batches from them, and solved windows would skip most of their linearisations
    bench.dump_outputs(str(tmp_path / "inproc"), batch, keep)
    c = {f[:-4]: np.load(str(tmp_path / "inproc" / f)) for f in os.listdir(str(tmp_path / "inproc"))}
    assert sorted(c) == sorted(a)
    for k in a:
        assert rel(c[k], a[k]) < 1e-12, k
    for k in range(B):
        assert np.array_equal(Wm[k].pose, np.asarray(wins[k]["pose"], float)) and np.array_equal(Wm[k].sb, np.asarray(wins[k]["speedbias"], float))
        assert np.array_equal(Wm[k].ex, np.asarray(wins[k]["ex_pose"], float).reshape(Wm[k].ex.shape)) and np.array_equal(Wm[k].lam, np.asarray(wins[k]["lam"], float))
        assert keep[1][k].pose is Wm[k].pose
    batch.synchronize(); batch.download_states()
    s = batch.summaries()
    assert rel(a["pose"], np.stack([w.pose for w in Wm])) < 1e-12 and rel(a["speedbias"], np.stack([w.sb for w in Wm])) < 1e-12
    assert rel(a["inv_depth"], np.stack([w.lam for w in Wm])) < 1e-12 and rel(a["ex_pose"], np.stack([w.ex for w in Wm])) < 1e-12
    assert "td" not in a and not np.array_equal(a["pose"][0], np.asarray(wins[0]["pose"], float))
    assert rel(a["final_cost"], [s[k].final_cost for k in range(B)]) < 1e-12 and np.all(a["final_cost"] < a["initial_cost"])
    for i in (0, len(ps) // 2, len(ps) - 1):
        P = batch.prior(int(ps[i]))
        m, n, _nb, xs = P.dims()
        As, bs = P.schur()
        d = P.export()
        assert tuple(a["prior_dims"][i]) == (m, n)
        assert rel(a["prior_A"][i, :n, :n], As) < 1e-12 and rel(a["prior_b"][i, :n], bs) < 1e-12
        assert rel(a["prior_J0"][i, :n, :n], d["J0"]) < 1e-12 and rel(a["prior_r0"][i, :n], d["r0"]) < 1e-12
        assert rel(a["prior_x0"][i, :xs], np.concatenate([np.atleast_1d(x) for x in d["x0"]])) < 1e-12
        J0 = a["prior_J0"][i, :n, :n]
        assert fro(J0.T @ J0, As) < 1e-6          # the prior the next frame takes: J0^T J0 = A'
