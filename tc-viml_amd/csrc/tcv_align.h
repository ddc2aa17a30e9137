// Layout shared by the alignment kernels (tcv_align.hip) and their host half (tcv_align_host.cpp): include/tcv_vi_alignment.h.
#pragma once
#include <stddef.h>

namespace tcv {

enum {
    AL_THREADS = 64,      // one wavefront per sequence: the factorisation is a chain of 3 F dependent steps, the wave's lanes share each step
    AL_BW = 5,            // scalar half-bandwidth of the velocity block (two neighbouring frames: 3 + 3 unknowns)
    AL_BANDW = AL_BW + 1, // band row r holds A(r, r - 5 .. r) at [0 .. 5]
    AL_NB = 4,            // border unknowns of LinearAlignment [g 3 | 100 s]; RefineGravity uses [dg 2 | 100 s]: vectors 0, 1 and 3
    AL_NVEC = AL_NB + 1,  // the border rows and the right-hand side, pushed through the band factor together
    AL_REC = 40,          // per-interval record in LDS: dt | Ri' Rj 9 | border columns of tmp_A 6 x 4 | tmp_b 6
    AL_BIAS_IN = 13,      // per interval into the bias kernel: jacobian.block<3,3>(O_R, O_BG) row-major 9 | delta_q xyzw 4
    AL_BIAS_OUT = 5,      // per sequence out of it: delta_bg 3 | status | smallest relative pivot
    AL_PRE_IN = 7,        // per interval into the alignment kernel: delta_p 3 | delta_v 3 | sum_dt
    AL_HEAD = 24,         // head of a sequence's output record (below)
};

// One sequence of a batch; the offsets count doubles (ints for o_key) from the start of their pools.
struct AlignHdr {
    int n_frames, n_key;
    int o_frame;      // R: 9 doubles per frame at 9 * o_frame, T: 3 per frame at 3 * o_frame (pools of their own)
    int o_itv;        // the sequence's first interval: per-interval inputs at AL_BIAS_IN * o_itv / AL_PRE_IN * o_itv
    int o_key;        // key_frame ints
    int status_in;    // alignment kernel: the bias kernel's status (not 0: the sequence is skipped)
    long long o_out;  // output record of the alignment kernel, doubles
    double tic[3];
};

// Output record of the alignment kernel: head | velocity 3 F | Ps 3 K | Rs 9 K | Vs 3 K
//   head: status | scale | gravity_c0 3 | gravity 3 | rot_diff 9 | smallest relative pivot | 0 ...
inline long long align_out_doubles(int F, int K) { return AL_HEAD + 3LL * F + 15LL * K; }

// dynamic LDS of the alignment kernel for sequences of up to F frames, doubles: band | its diagonal before elimination | the border rows and
// the right-hand side | records | misc 64.  F = 128: 78 KB
inline size_t align_lds_doubles(int F) {
    const size_t n = 3 * (size_t)F;
    return n * AL_BANDW + n + AL_NVEC * (n + AL_NB) + (size_t)AL_REC * (F - 1) + 64;
}

struct AlignOpts { double gravity_norm, min_relative_pivot; };

}  // namespace tcv

extern "C" int tcv_launch_align_bias(int n, const tcv::AlignHdr *hdrs, const double *R, const double *itv, double *out, double min_relative_pivot, void *stream);
extern "C" int tcv_launch_align_solve(int n, const tcv::AlignHdr *hdrs, const double *R, const double *T, const double *itv, const int *keys, double *out,
                                      tcv::AlignOpts opts, size_t lds_bytes, void *stream);
