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
