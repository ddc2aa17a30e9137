"""Seeded inputs of the visual-inertial alignment tests, on synth.py's analytic trajectory (no trajectory code of their own): F frames at a
period of 10 or 20 IMU samples, the body poses expressed in a random SfM frame at a random scale, IMU samples from traj_a / traj_w_body
with a true gyroscope bias and optional noise, and a key-frame subset.  `truth` holds what the alignment has to recover."""
import numpy as np

import synth

NOISE = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
BG_TRUE = np.array([0.01, -0.02, 0.015])


def _random_rotation(rng):
    q = rng.normal(size=4)
    return synth.q2R(q / np.linalg.norm(q))


def make_case(seed, n_frames, period=20, noisy=False, key="all", scale=None, bg_true=BG_TRUE):
    """period: IMU samples per frame interval (20: 100 ms frames, 10: 50 ms).  key: "all", "sparse" (every third frame and the last) or "one"."""
    rng = np.random.default_rng(seed)
    F, S, dt = n_frames, period, synth.DT_IMU
    t0 = rng.uniform(0.0, 6.0)
    ts = t0 + dt * np.arange((F - 1) * S + 1)
    tf = ts[::S]
    Rwb, pw = synth.traj_R(tf), synth.traj_p(tf)
    g_w = np.array([0.0, 0.0, synth.G_NORM])
    acc = np.einsum("tji,tj->ti", synth.traj_R(ts), synth.traj_a(ts) + g_w)      # R' (a + g): un_acc = R (acc - ba) - g
    gyr = synth.traj_w_body(ts) + bg_true
    if noisy:
        acc = acc + rng.normal(scale=synth.ACC_N, size=acc.shape); gyr = gyr + rng.normal(scale=synth.GYR_N, size=gyr.shape)
    Rc0 = _random_rotation(rng)
    sc = float(rng.uniform(0.4, 4.0)) if scale is None else float(scale)
    tic = synth.TIC.copy()
    pc = pw + np.einsum("tij,j->ti", Rwb, tic)                                   # camera positions in the world
    T = (pc - pc[0]) @ Rc0.T / sc                                                # ImageFrame::T: up to scale, in the SfM frame
    R = np.einsum("ij,tjk->tik", Rc0, Rwb)                                       # ImageFrame::R: body rotation in the SfM frame
    imu = []
    for i in range(F - 1):
        k = i * S
        imu.append((acc[k].copy(), gyr[k].copy(), np.concatenate([np.full((S, 1), dt), acc[k + 1:k + S + 1], gyr[k + 1:k + S + 1]], 1)))
    if key == "all":
        kf = np.arange(F)
    elif key == "sparse":
        kf = np.unique(np.concatenate([np.arange(0, F, 3), [F - 1]]))
    else:
        kf = np.array([F // 2])
    ba0 = rng.normal(scale=1e-3, size=3) if seed % 2 else np.zeros(3)
    bg0 = rng.normal(scale=1e-3, size=3) if seed % 3 == 0 else np.zeros(3)
    vb = np.einsum("tji,tj->ti", Rwb, synth.traj_v(tf))                          # body-frame velocities
    return dict(name="F%d_S%d_%s%s_seed%d" % (F, S, key, "_noisy" if noisy else "", seed), R=R, T=T, tic=tic, imu=imu, ba0=ba0, bg0=bg0, noise=NOISE,
                key_frame=kf.astype(np.int32), period=S, acc=acc, gyr=gyr,
                truth=dict(scale=sc, gravity_c0=Rc0 @ g_w, bg=np.asarray(bg_true, dtype=np.float64), velocity=vb))


def imu_arrays(case):
    """(acc, gyr, dt) as synth.preintegrate / tcv.preintegrate take them: (F - 1, S + 1, 3) with sample 0 taken at the start frame"""
    S = case["period"]
    n = len(case["imu"])
    idx = np.arange(n)[:, None] * S + np.arange(S + 1)[None, :]
    return case["acc"][idx], case["gyr"][idx], synth.DT_IMU


def run_oracle(case, preintegrate, dtype=np.float64, gate=0.0, gravity_norm=9.81007, T=None):
    """the restatement end to end: `preintegrate(acc, gyr, dt, ba, bg)` is synth.preintegrate or a wrapper of tcv.preintegrate.  Returns
    (result dict of vi_alignment_oracle.align + delta_bg / bg / bias_pivots, the re-propagated pre-integrations)"""
    import vi_alignment_oracle as VO
    acc, gyr, dt = imu_arrays(case)
    pre0 = preintegrate(acc, gyr, dt, case["ba0"], case["bg0"])
    dbg, piv = VO.gyro_bias(case["R"], pre0, dtype, gate)
    bg = case["bg0"] + np.asarray(dbg, dtype=np.float64)      # what the host adds (initial_aligment.cpp:29-30)
    pre1 = preintegrate(acc, gyr, dt, np.zeros(3), bg)
    out = VO.align(case["R"], case["T"] if T is None else T, case["tic"], pre1, case["key_frame"], gravity_norm, dtype, gate)
    out.update(delta_bg=dbg, bg=bg, bias_pivots=piv)
    return out, pre1


# the frame counts of the GPU tests: the issue's list, the singular pair, and the neighbours of the sizes built into the kernel --
#   AL_THREADS = 64 lanes: 3 F = 63 | 66 unknowns (F = 21, 22), F - 1 = 63 | 64 | 65 intervals (F = 64, 65, 66), F = 63 | 64 | 65 frames and key frames
#   TCV_VI_ALIGN_MAX_FRAMES = 128 (F = 127, 128)
GPU_FRAMES = (4, 5, 11, 21, 22, 63, 64, 65, 66, 127, 128)


def gpu_cases():
    """one well-posed case per frame count, alternating the frame period and the key-frame subset; n_key = 1 twice"""
    out = []
    for k, F in enumerate(GPU_FRAMES):
        # (four frames need the 50 ms period's geometry no more than the 100 ms one's; both are measured well-posed in test_vi_alignment_cpu.py)
        out.append(make_case(100 + k, F, period=(20, 10)[k % 2], key=("all", "sparse", "all", "one")[k % 4]))
    out.append(make_case(150, 11, period=10, key="one", noisy=True))
    out.append(make_case(151, 12, period=20, key="sparse", noisy=True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs off the well-posed path (tests/test_vi_alignment_cpu.py decides on the restatement alone that each is decisive; then
# tests/test_gpu_vi_alignment_paths.py and tests/dev/fuzz_vi_alignment.py run them on the device).  These carry their IMU stream only as the
# `imu` list -- counts and dt may differ inside a sequence -- so they go through run_oracle_imu, not run_oracle.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _Ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _assemble(name, ts, fidx, Rwb_f, pw_f, vw_f, acc, gyr, Rc0, sc, kf, ba0=None, bg0=None, noise=NOISE, bg_true=None, T=None, dts=None):
    """a case from samples `acc`, `gyr` at the times `ts` (sample k + 1 is pushed with dt = dts[k], ts[k + 1] - ts[k] up to rounding) and the frames
    at ts[fidx]"""
    F = len(fidx)
    tic = synth.TIC.copy()
    pc = pw_f + np.einsum("tij,j->ti", Rwb_f, tic)
    if T is None:
        T = (pc - pc[0]) @ Rc0.T / sc
    R = np.einsum("ij,tjk->tik", Rc0, Rwb_f)
    dts = np.full(len(ts) - 1, synth.DT_IMU) if dts is None else dts
    imu = [(acc[fidx[i]].copy(), gyr[fidx[i]].copy(), np.concatenate([dts[fidx[i]:fidx[i + 1], None], acc[fidx[i] + 1:fidx[i + 1] + 1], gyr[fidx[i] + 1:fidx[i + 1] + 1]], 1))
           for i in range(F - 1)]
    g_w = np.array([0.0, 0.0, synth.G_NORM])
    return dict(name=name, R=R, T=T, tic=tic, imu=imu, ba0=np.zeros(3) if ba0 is None else ba0, bg0=np.zeros(3) if bg0 is None else bg0, noise=tuple(noise),
                key_frame=np.asarray(kf, dtype=np.int32),
                truth=dict(scale=sc, gravity_c0=Rc0 @ g_w, bg=np.zeros(3) if bg_true is None else np.asarray(bg_true, dtype=np.float64),
                           velocity=np.einsum("tji,tj->ti", Rwb_f, vw_f)))


def _on_synth_trajectory(name, ts, fidx, Rc0, sc, kf, bg_true=BG_TRUE, rng=None, noisy=False, **kw):
    g_w = np.array([0.0, 0.0, synth.G_NORM])
    acc = np.einsum("tji,tj->ti", synth.traj_R(ts), synth.traj_a(ts) + g_w)
    gyr = synth.traj_w_body(ts) + bg_true
    if noisy:
        acc = acc + rng.normal(scale=synth.ACC_N, size=acc.shape); gyr = gyr + rng.normal(scale=synth.GYR_N, size=gyr.shape)
    tf = ts[fidx]
    return _assemble(name, ts, fidx, synth.traj_R(tf), synth.traj_p(tf), synth.traj_v(tf), acc, gyr, Rc0, sc, kf, bg_true=bg_true, **kw)


def _vertical(name, F, period, Rc0, sc=2.0):
    """no rotation, motion along z only: z(t) = 0.4 sin(1.3 t) + 0.15 sin(3.1 t + 0.5).  Gyroscope exactly 0, accelerometer exactly (0, 0, z'' + G)."""
    ts = 0.7 + synth.DT_IMU * np.arange((F - 1) * period + 1)
    fidx = np.arange(F) * period
    z = 0.4 * np.sin(1.3 * ts) + 0.15 * np.sin(3.1 * ts + 0.5)
    vz = 0.4 * 1.3 * np.cos(1.3 * ts) + 0.15 * 3.1 * np.cos(3.1 * ts + 0.5)
    az = -0.4 * 1.69 * np.sin(1.3 * ts) - 0.15 * 9.61 * np.sin(3.1 * ts + 0.5)
    zero = np.zeros_like(ts)
    acc = np.stack([zero, zero, az + synth.G_NORM], 1)
    I = np.broadcast_to(np.eye(3), (F, 3, 3)).copy()
    return _assemble(name, ts, fidx, I, np.stack([zero, zero, z], 1)[fidx], np.stack([zero, zero, vz], 1)[fidx], acc, np.zeros_like(acc), Rc0, sc, np.arange(F))


def vertical_case(F, period, sign):
    """gravity exactly along +z (sign = +1: Rc0 = I) or -z (sign = -1: Rc0 = diag(1, -1, -1)) of the SfM frame: Ri' Rj is exactly I, the x / y rows
    of every system have an exactly zero right-hand side, gravity_c0 comes out as (+-0, +-0, +-G) exactly"""
    assert sign in (1, -1)
    return _vertical("vertical_F%d_S%d_%s" % (F, period, "up" if sign > 0 else "down"), F, period, np.diag([1.0, float(sign), float(sign)]))


def tilted_case(F, period, delta):
    """vertical_case(sign = -1) with Rc0 rotated by `delta` about y on top: gravity `delta` away from -z"""
    return _vertical("tilted_F%d_S%d_%g" % (F, period, delta), F, period, _Ry(delta) @ np.diag([1.0, -1.0, -1.0]))


def stationary_case(F, period=20):
    """a camera at rest: T == 0 exactly (the scale column is zero), the accelerometer reads gravity in the body, the gyroscope its bias"""
    ts = synth.DT_IMU * np.arange((F - 1) * period + 1)
    fidx = np.arange(F) * period
    Rb = synth.traj_R(np.array([1.3]))[0]
    acc = np.tile(Rb.T @ np.array([0.0, 0.0, synth.G_NORM]), (len(ts), 1))
    gyr = np.tile(BG_TRUE, (len(ts), 1))
    Rc0 = _random_rotation(np.random.default_rng(F))
    c = _assemble("stationary_F%d" % F, ts, fidx, np.tile(Rb, (F, 1, 1)), np.zeros((F, 3)), np.zeros((F, 3)), acc, gyr, Rc0, 1.0, np.arange(F), bg_true=BG_TRUE,
                  T=np.zeros((F, 3)))
    return c


def constant_velocity_case(F, period=20):
    """no rotation, no acceleration: scale and a common velocity are confounded (rank deficient by one, up to rounding)"""
    ts = synth.DT_IMU * np.arange((F - 1) * period + 1)
    fidx = np.arange(F) * period
    Rb = synth.traj_R(np.array([0.4]))[0]
    v = np.array([0.7, -0.4, 0.2])
    acc = np.tile(Rb.T @ np.array([0.0, 0.0, synth.G_NORM]), (len(ts), 1))
    gyr = np.tile(BG_TRUE, (len(ts), 1))
    Rc0 = _random_rotation(np.random.default_rng(100 + F))
    return _assemble("constant_velocity_F%d" % F, ts, fidx, np.tile(Rb, (F, 1, 1)), ts[fidx, None] * v[None, :], np.tile(v, (F, 1)), acc, gyr, Rc0, 1.5, np.arange(F),
                     bg_true=BG_TRUE)


def zero_dt_case(F, period=10):
    """every IMU sample pushed with dt == 0 (finite, so validated): the bias Jacobians are exactly zero and solveGyroscopeBias's first pivot fails
    on A_00 == 0 -- the one validated input that stops in the bias kernel and takes the alignment kernel's early exit"""
    c = make_case(40 + F, F, period)
    out = dict(c, name="zero_dt_F%d" % F, imu=[(a0, g0, np.concatenate([np.zeros((len(s), 1)), s[:, 1:]], 1)) for a0, g0, s in c["imu"]])
    del out["period"], out["acc"], out["gyr"]
    return out


def negated_T_case():
    """make_case(18, 11, 20) with T negated: LinearAlignment's s is the true scale with a minus sign, status 1 by `s < 0` (:184)"""
    c = make_case(18, 11, 20)
    out = dict(c, name="negated_T", T=-c["T"])
    del out["period"], out["acc"], out["gyr"]
    return out


def huge_acc_case(k, kT=100):
    """make_case(18, 11, 20) with every accelerometer value x 10^k and T x 10^kT, all finite.  The matrices do not see the accelerometer, so the
    rank gate passes; the right-hand side does (delta_p, delta_v), and its products with the scale column overflow float64 from k + kT near
    309: the route to status 4 after LinearAlignment.  Below that the solution is finite with |g| ~ 10^k: status 1."""
    c = make_case(18, 11, 20)
    f = 10.0 ** k
    out = dict(c, name="acc_1e%d_T_1e%d" % (k, kT), T=c["T"] * 10.0 ** kT,
               imu=[(a0 * f, g0, np.concatenate([s[:, :1], s[:, 1:4] * f, s[:, 4:]], 1)) for a0, g0, s in c["imu"]])
    del out["period"], out["acc"], out["gyr"]
    return out


def noise_T_case(seed, F, period=20, sigma=1.0):
    """make_case with T replaced by seeded noise that knows nothing of the motion: the scale estimate is near zero, with a random sign"""
    c = make_case(seed, F, period)
    rng = np.random.default_rng(9000 + seed)
    out = dict(c, name="noise_T_F%d_seed%d" % (F, seed), T=rng.normal(scale=sigma, size=(F, 3)))
    del out["period"], out["acc"], out["gyr"]
    return out


def ragged_case(seed, F):
    """per-interval sample counts from 3 .. 40, per-sample dt from {2.5, 5, 10} ms (the trajectory sampled at the resulting times), a random
    key-frame subset without frame 0"""
    rng = np.random.default_rng(7000 + seed)
    counts = rng.integers(3, 41, size=F - 1)
    fidx = np.concatenate([[0], np.cumsum(counts)])
    dts = rng.choice([0.0025, 0.005, 0.01], size=fidx[-1])
    ts = rng.uniform(0.0, 6.0) + np.concatenate([[0.0], np.cumsum(dts)])
    nk = int(rng.integers(1, F))
    kf = np.sort(rng.choice(np.arange(1, F), size=nk, replace=False))
    return _on_synth_trajectory("ragged_F%d_seed%d" % (F, seed), ts, fidx, _random_rotation(rng), float(rng.uniform(0.4, 4.0)), kf,
                                ba0=rng.normal(scale=1e-3, size=3), bg0=rng.normal(scale=1e-3, size=3), dts=dts)


NOISE_B = (2.0 * synth.ACC_N, 0.5 * synth.GYR_N, 3.0 * synth.ACC_W, synth.GYR_W)      # a second noise vector, for the batches that mix two


def fuzz_case(seed):
    """one draw of tests/dev/fuzz_vi_alignment.py: F 4 .. 40, uniform or ragged periods in 5 .. 25, dt uniform or per sample, key frames all /
    sparse / one / random, IMU noise on or off, scale log-uniform in 0.05 .. 50, gyroscope bias up to 0.1 rad/s, Rc0 random or tilted within
    {0, 1e-7, 1e-3, 0.1} rad of +-z"""
    rng = np.random.default_rng(310000 + seed)
    F = int(rng.integers(4, 41))
    counts = rng.integers(5, 26, size=F - 1) if rng.random() < 0.5 else np.full(F - 1, int(rng.integers(5, 26)))
    fidx = np.concatenate([[0], np.cumsum(counts)])
    dts = rng.choice([0.0025, 0.005, 0.01], size=fidx[-1]) if rng.random() < 0.5 else np.full(fidx[-1], float(rng.choice([0.005, 0.01])))
    ts = rng.uniform(0.0, 6.0) + np.concatenate([[0.0], np.cumsum(dts)])
    kind = str(rng.choice(["all", "sparse", "one", "random"]))
    if kind == "all":
        kf = np.arange(F)
    elif kind == "sparse":
        kf = np.unique(np.concatenate([np.arange(0, F, 3), [F - 1]]))
    elif kind == "one":
        kf = np.array([int(rng.integers(0, F))])
    else:
        kf = np.sort(rng.choice(np.arange(F), size=int(rng.integers(1, F + 1)), replace=False))
    noisy = bool(rng.random() < 0.5)
    sc = float(np.exp(rng.uniform(np.log(0.05), np.log(50.0))))
    bg_true = rng.uniform(-0.1, 0.1, size=3)
    if rng.random() < 0.5:
        Rc0, frame = _random_rotation(rng), "random"
    else:
        sign, delta = float(rng.choice([1.0, -1.0])), float(rng.choice([0.0, 1e-7, 1e-3, 0.1]))
        # (the trajectory's own attitude keeps Ri' Rj away from I: gravity is exactly on the axis only up to rounding)
        Rc0, frame = _Ry(delta) @ np.diag([1.0, sign, sign]), "%sz+%g" % ("+" if sign > 0 else "-", delta)
    name = "fuzz%d_F%d_%s_%s_%s%s_sc%.2g" % (seed, F, "ragged" if len(set(counts)) > 1 else "S%d" % counts[0], kind, frame, "_noisy" if noisy else "", sc)
    return _on_synth_trajectory(name, ts, fidx, Rc0, sc, kf, bg_true=bg_true, rng=rng, noisy=noisy, noise=NOISE if rng.random() < 0.7 else NOISE_B, dts=dts)


# The committed inputs of the path tests, found on the restatement alone (tests/test_vi_alignment_cpu.py asserts each of them there):
DEFAULT_GATE = 4e-11      # tcv_vi_align_options_default
VERTICAL = [(F, S, sign) for F, S in ((4, 10), (11, 10)) for sign in (1, -1)]
TILTED = [(11, 10, 1e-7), (4, 10, 1e-7), (11, 10, 1e-2), (4, 10, 1e-2)]
# noise_T_case (seed, F) on which float64 and long double both end in REFINED_SCALE (searched over seeds 0 .. 39 at F = 5, 8, 11, 16: 32 hits)
STATUS2 = [(2, 5), (5, 5), (9, 5), (2, 8), (12, 11), (15, 11)]
# (F, period of make_case(7 + F, F, period), min_relative_pivot, site): the gate in the geometric middle of two neighbouring recorded pivots
# >= 30^2 apart, the site where the first failing pivot falls
RANK_SITES = [(4, 10, 1.74e-6, "linear border"), (5, 10, 5.43e-6, "linear border")]
SINGULAR_FRAMES = (4, 5, 11, 22)
# huge_acc_case(k, 100): the float64 restatement turns from LINEAR (finite) to NON_FINITE between k = 208 and 209; two decades on each side
NON_FINITE_K, LINEAR_SIDE_K = 212, 206


def preint_np(imu, ba, bg):
    """the pre-integrations of an `imu` list on the CPU, in the dict layout of synth.preintegrate: synth.preintegrate where counts and dt are
    uniform, np_oracle.preintegrate (which takes one dt per sample) interval by interval where they are not.  (Both at NOISE: the alignment reads
    delta_p, delta_q, delta_v and the Jacobian, never the covariance.)"""
    import np_oracle
    counts = {len(m[2]) for m in imu}
    dts = {float(v) for m in imu for v in m[2][:, 0]}
    if len(counts) == 1 and len(dts) == 1:
        acc = np.stack([np.concatenate([m[0][None], m[2][:, 1:4]]) for m in imu]); gyr = np.stack([np.concatenate([m[1][None], m[2][:, 4:7]]) for m in imu])
        return synth.preintegrate(acc, gyr, dts.pop(), np.asarray(ba, dtype=np.float64), np.asarray(bg, dtype=np.float64))
    rs = [np_oracle.preintegrate(np.concatenate([m[0][None], m[2][:, 1:4]]), np.concatenate([m[1][None], m[2][:, 4:7]]), m[2][:, 0], np.asarray(ba, dtype=np.float64),
                                 np.asarray(bg, dtype=np.float64), *NOISE) for m in imu]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in rs[0]}


def preint_tcv(tcv, imu, ba, bg, noise):
    """tcv_preintegrate on an `imu` list (ragged counts, per-sample dt) in one call, in the dict layout of tcv.preintegrate"""
    import tcv_vi_alignment as va
    n = len(imu)
    count = tcv.i32([len(m[2]) for m in imu])
    first = tcv.i32(np.concatenate([[0], np.cumsum(count)[:-1]]))
    samples = tcv.f64(np.concatenate([m[2] for m in imu]))
    init = tcv.f64(np.array([np.concatenate([m[0], m[1], ba, bg]) for m in imu]))
    out = (tcv.ImuPreintegration * n)()
    tcv.check(tcv.lib().tcv_preintegrate(n, tcv.iptr(first), tcv.iptr(count), tcv.dptr(samples), len(samples), tcv.dptr(init), tcv.dptr(tcv.f64(noise)), out))
    return va.preint_dict(out, n)


def run_oracle_imu(case, preintegrate=preint_np, dtype=np.float64, gate=0.0, gravity_norm=9.81007, solver="cholesky", pre0=None, pre1=None):
    """run_oracle for a case that carries its stream as the `imu` list, with the verdicts and zero patterns of the header: `preintegrate(imu,
    ba, bg)`; `pre0` / `pre1` given: those pre-integrations instead (the device's own).  Adds delta_bg, bg, bias_status, bias_pivots, and
    min_pivot: the smallest relative pivot that PASSED the gate, capped at 1, what tcv_vi_align_result::min_pivot records."""
    import vi_alignment_oracle as VO
    if pre0 is None:
        pre0 = preintegrate(case["imu"], case["ba0"], case["bg0"])
    F, K = len(case["R"]), len(case["key_frame"])
    if solver == "dense":
        sb, dbg, bpiv, ba0 = VO.OK, VO.gyro_bias(case["R"], pre0, dtype, solver="dense")[0], np.ones(0), None
    else:
        sb, dbg, bpiv, ba0 = VO.gyro_bias_verdict(case["R"], pre0, dtype, gate)
    if sb != VO.OK:
        out = dict(status=sb, scale=dtype(0), gravity_c0=np.zeros(3, dtype), gravity=np.zeros(3, dtype), rot_diff=np.zeros((3, 3), dtype), velocity=np.zeros((F, 3), dtype),
                   Ps=np.zeros((K, 3), dtype), Rs=np.zeros((K, 3, 3), dtype), Vs=np.zeros((K, 3), dtype), pivots=np.ones(0, dtype), stages=[], fail_a0=ba0, flags={},
                   delta_bg=np.zeros(3, dtype), bg=np.zeros(3), bias_status=sb, bias_pivots=bpiv, min_pivot=1.0, site="bias")
        return out, None
    bg = case["bg0"] + np.asarray(dbg, dtype=np.float64)
    if pre1 is None:
        pre1 = preintegrate(case["imu"], np.zeros(3), bg)
    out = VO.align(case["R"], case["T"], case["tic"], pre1, case["key_frame"], gravity_norm, dtype, gate, solver)
    out.update(delta_bg=dbg, bg=bg, bias_status=sb, bias_pivots=bpiv)
    passed = [float(p) for p in bpiv] + [float(p) for _, piv in out["stages"] for p in piv]
    if out["status"] == VO.RANK:
        passed = passed[:-1]
        stage, piv = out["stages"][-1]
        out["site"] = ("band" if len(piv) <= 3 * F else "linear border" if stage == "linear" else "refine border")
    out["min_pivot"] = min([1.0] + passed)
    return out, pre1
