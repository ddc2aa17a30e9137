// Process-level runtime under every entry point (tcv_runtime.cpp): the thread-local error text, the device free list, the pinned staging
// pool, the calling thread's streams and the guards that tie one call's buffers to the stream its commands run on.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tcv.h"

namespace tcv {
// device allocations go through a per-process free list (size-bucketed, per device): a per-frame estimator creates and destroys a
// batch every frame, and hipMalloc / hipFree (each a device synchronisation) were a quarter of its host time
hipError_t dev_malloc(void **p, size_t bytes);
hipError_t dev_free(void *p);
long long dev_pool_misses();
void dev_pool_stats(unsigned long long *live_bytes, unsigned long long *cached_bytes, int *live_buffers);
int hip_fail(hipError_t e, const char *what);
int device_ready();
void set_error(const std::string &s);
#define HIPCHK(x)                                              \
    do {                                                       \
        hipError_t e_ = (x);                                   \
        if (e_ != hipSuccess) return tcv::hip_fail(e_, #x);    \
    } while (0)
// pinned host staging buffers for uploads / downloads, recycled through a small per-process pool (hipHostMalloc costs milliseconds)
void *host_staging_acquire(size_t bytes);
void host_staging_release(void *p);
// buffers of commands left in flight on the calling thread's stream `st`: released at the thread's next wait on it (tcv_runtime.cpp)
void defer_release(void *host_staging, void *dev_buf, hipStream_t st);
void flush_deferred(hipStream_t st);
hipError_t stream_wait(hipStream_t st);      // waits for the stream; for the device when `st` is the null stream
// The buffers of ONE call's transfer: a pinned staging buffer and, optionally, one pooled device buffer, bound to the stream the call's
// commands go to.  Both go back to process-wide pools that other host threads take from, so releasing them while a copy or a kernel on
// `st` still uses them is a use-after-free across threads: once the call has said issued(), every exit waits for the stream first.
struct StagedTransfer {
    void *host, *dev = nullptr;
    const hipStream_t st;
    StagedTransfer(hipStream_t stream, size_t host_bytes) : host(host_staging_acquire(host_bytes)), st(stream) {}
    StagedTransfer(const StagedTransfer &) = delete;
    ~StagedTransfer();                                      // in flight: waits for the stream; then both buffers go back to their pools
    hipError_t dev_alloc(size_t bytes) { return dev_malloc(&dev, bytes); }
    void issued() { in_flight = true; }                     // a command that uses a buffer is on the stream, or about to be
    hipError_t wait();                                      // no longer in flight once a wait has succeeded
    void park();                                            // left in flight: the buffers are released at the thread's next wait on the stream (defer_release)
    void *take_dev() { void *p = dev; dev = nullptr; return p; }      // the caller keeps the device buffer (and frees it behind this guard's wait)
private:
    bool in_flight = false;
};
// blocking download through pinned staging on the calling thread's own stream (the default stream serialises the host threads of a process)
int staged_download(void *dst, const void *d_src, size_t bytes, const char *what);
// the other direction, same contract: `bytes` of host memory into device memory, TCV_OK or the hip_fail status under `what`
int staged_upload(void *d_dst, const void *src, size_t bytes, const char *what);
// a non-blocking stream of the calling thread on its current device, created on first use and kept: the one-shot entry points
// (pre-integration, line association, gauge fix, the factor evaluators) launch there and wait for THAT stream, never for the device --
// another host thread's batches keep running (several estimator groups per GPU, bench.py --mode replay)
hipStream_t util_stream();
// the stream argument of an asynchronous entry point (include/tcv.h): TCV_STREAM_THREAD is the calling thread's stream, anything else a hipStream_t
inline hipStream_t resolve_stream(void *hip_stream) { return hip_stream == TCV_STREAM_THREAD ? util_stream() : (hipStream_t)hip_stream; }
// the calling thread's second stream (created at first use): the native estimator runs a frame's marginalisation there, beside the next
// frame's association and upload on the thread's main stream
hipStream_t aux_stream();

// One call's round trip: arrays up, the caller's kernel(s), results down, one wait -- all on the stream of the StagedTransfer that owns the
// buffers, which is also what makes every error exit behind issued() wait before they return to their pools.
//   pinned staging  [inputs | outputs]
//   device buffer   [inputs | outputs | device-only scratch]
// The regions lie back to back, each rounded up to 8 bytes.  `inout` bytes at the end of the inputs are at the same time the head of
// the outputs (a kernel that updates an array in place: they go up with the inputs and come back with the outputs).
struct RoundTrip {
    RoundTrip(hipStream_t stream, size_t in_bytes, size_t out_bytes, size_t scratch_bytes = 0, size_t inout = 0)
        : n_in(up8(in_bytes)), n_out(up8(out_bytes)), o_out(n_in - inout), tr(stream, o_out + n_out) {
        if (tr.host) alloc = tr.dev_alloc(o_out + n_out + scratch_bytes);
    }
    // TCV_OK, or why the call has no buffers; the regions may be touched only after TCV_OK
    int ready(const char *what) const {
        if (!tr.host) { set_error(std::string("hipHostMalloc (staging) failed: ") + what); return TCV_ERR_HIP; }
        return alloc == hipSuccess ? (int)TCV_OK : hip_fail(alloc, what);
    }
    template <class T = double> T *h_in() const { return (T *)tr.host; }
    template <class T = double> T *h_out() const { return (T *)((char *)tr.host + o_out); }
    template <class T = double> T *d_in() const { return (T *)tr.dev; }
    template <class T = double> T *d_out() const { return (T *)((char *)tr.dev + o_out); }
    template <class T = double> T *d_scratch() const { return (T *)((char *)tr.dev + o_out + n_out); }
    // upload of the inputs, launch(stream), download of the outputs, wait; TCV_OK or the hip_fail status under `what`
    template <class Launch> int run(const char *what, Launch &&launch) {
        tr.issued();
        hipError_t e = hipMemcpyAsync(tr.dev, tr.host, n_in, hipMemcpyHostToDevice, tr.st);
        if (e == hipSuccess) { launch(tr.st); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipMemcpyAsync(h_out<char>(), d_out<char>(), n_out, hipMemcpyDeviceToHost, tr.st);
        if (e == hipSuccess) e = tr.wait();
        return e == hipSuccess ? (int)TCV_OK : hip_fail(e, what);
    }
private:
    static size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }
    const size_t n_in, n_out, o_out;
    StagedTransfer tr;
    hipError_t alloc = hipSuccess;
};
}  // namespace tcv
