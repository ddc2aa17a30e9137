// Process-level runtime of the library (tcv_runtime.h): the calling thread's error text, the device free list, the pinned staging pool,
// the per-thread streams and their park, deferred releases, StagedTransfer / staged_download / staged_upload, and the small entry points of include/tcv.h
// that concern the process rather than a problem or a batch.  There is no CPU fallback: without a HIP device device_ready() says so.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#if defined(__linux__)
#include <sys/syscall.h>
#include <unistd.h>
#endif

#include "tcv_runtime.h"

namespace tcv {
static thread_local std::string g_err;
void set_error(const std::string &s) { g_err = s; }
int hip_fail(hipError_t e, const char *what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return TCV_ERR_HIP;
}
// ---- device memory free list -------------------------------------------------------------------------------------------------
namespace {
struct DevPool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> free_list;      // (device, bucket bytes) -> buffer
    std::map<void *, std::pair<int, size_t>> live;               // buffer -> (device, bucket bytes)
    size_t cached = 0;
};
DevPool &pool() { static DevPool *p = new DevPool(); return *p; }      // leaked on purpose: no hipFree at process exit after the runtime is gone
size_t bucket_of(size_t n) {
    if (n <= 256) return 256;
    if (n > (size_t(2) << 20)) return (n + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);      // 2 MiB granules above 2 MiB
    size_t b = 256;
    while (b < n) b <<= 1;
    return b;
}
constexpr size_t POOL_MAX_CACHED = size_t(3) << 30;
}  // namespace
static std::atomic<long long> g_dev_misses{0};
long long dev_pool_misses() { return g_dev_misses.load(); }
hipError_t dev_malloc(void **p, size_t bytes) {
    static const bool off = getenv("TCV_NO_DEV_POOL") != nullptr;
    if (off) return ::hipMalloc(p, bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t b = bucket_of(bytes);
    DevPool &P = pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.free_list.find({dev, b});
        if (it != P.free_list.end()) { *p = it->second; P.free_list.erase(it); P.cached -= b; P.live[*p] = {dev, b}; return hipSuccess; }
    }
    g_dev_misses++;
    hipError_t e = ::hipMalloc(p, b);
    if (e != hipSuccess) {      // out of memory: give the cached buffers back and retry once
        std::vector<void *> drop;
        { std::lock_guard<std::mutex> g(P.mu); for (auto &kv : P.free_list) drop.push_back(kv.second); P.free_list.clear(); P.cached = 0; }
        for (void *q : drop) (void)::hipFree(q);
        e = ::hipMalloc(p, b);
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> g(P.mu);
    P.live[*p] = {dev, b};
    return hipSuccess;
}
hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    DevPool &P = pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.live.find(p);
        if (it != P.live.end()) {
            const auto key = it->second;
            P.live.erase(it);
            if (P.cached + key.second <= POOL_MAX_CACHED) { P.free_list.insert({key, p}); P.cached += key.second; return hipSuccess; }
        }
    }
    return ::hipFree(p);
}

void dev_pool_stats(unsigned long long *live_bytes, unsigned long long *cached_bytes, int *live_buffers) {
    DevPool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    unsigned long long lb = 0;
    for (auto &kv : P.live) lb += kv.second.second;
    if (live_bytes) *live_bytes = lb;
    if (cached_bytes) *cached_bytes = P.cached;
    if (live_buffers) *live_buffers = (int)P.live.size();
}

// The calling thread's own stream per device.  A host thread that ends gives its streams back: the runtime maps streams onto a handful of
// hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and a stream that is never destroyed keeps its share of a queue -- after a few
// generations of short-lived host threads two LIVE threads end up on one queue and the small commands of one (a pre-integration, an
// upload) wait behind the other's 2 ms solve kernel (lock-step replay on 2 host threads: 1 500 against 2 200 windows/s).  The main thread's
// streams are left to the runtime's own teardown at process exit.
namespace {
struct Deferred { void *h, *d; hipStream_t st; };
struct ThreadStreams {
    std::map<int, hipStream_t> m;
    std::map<int, hipStream_t> aux;      // a second stream per device for work that runs beside the thread's main sequence (aux_stream)
    std::vector<Deferred> deferred;      // buffers of commands still in flight on one of these streams (defer_release)
    bool main_thread = false;
    ~ThreadStreams();
};
ThreadStreams &thread_streams() { thread_local ThreadStreams mine; return mine; }
}  // namespace
// A call that leaves its commands in flight on the calling thread's stream (tcv_preintegrate_device: nobody on the host needs the result)
// parks the pinned staging buffer and the device input blob here instead of waiting for the stream; they go back to their pools at the
// thread's next wait on that stream (every tcv_batch_create ends with one).
// The list is bounded: a thread that pre-integrates and never creates a batch (or whose frames keep failing before tcv_batch_create) would
// otherwise pin host and device memory until it ends -- at DEFER_MAX parked commands the stream is drained and its buffers released.
enum { DEFER_MAX = 32 };
hipError_t stream_wait(hipStream_t st) { return st ? hipStreamSynchronize(st) : hipDeviceSynchronize(); }
void defer_release(void *host_staging, void *dev_buf, hipStream_t st) {
    std::vector<Deferred> &v = thread_streams().deferred;
    if (v.size() >= DEFER_MAX) { (void)stream_wait(st); flush_deferred(st); }
    v.push_back(Deferred{host_staging, dev_buf, st});
}
void flush_deferred(hipStream_t st) {
    std::vector<Deferred> &v = thread_streams().deferred;
    size_t k = 0;
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].st == st) { host_staging_release(v[i].h); (void)dev_free(v[i].d); }
        else v[k++] = v[i];
    }
    v.resize(k);
}
namespace {
// Streams of host threads that have ended, per device.  A thread's stream is drained and parked here instead of being destroyed: a batch
// that ran on it (TCV_STREAM_THREAD, the native estimator) may still hold the handle in BatchFlight::streams / last_stream, and a
// hipStreamSynchronize / hipEventRecord on a destroyed stream is an error (round-4 advisor finding).  The next new thread takes a parked
// stream over, so the process never holds more streams than it had live threads at once -- which is what keeps two LIVE threads off one
// hardware queue (see above).  Leaked on purpose, like the device pool.
// `orphans`: the buffers of commands a thread left in flight when it ended (defer_release), per stream; whoever takes the stream over waits
// for it once and releases them.  The destructor below makes NO HIP call: it runs among the thread's TLS destructors,
// where a profiler's own thread state may be gone already (rocprofv3 aborted in hipStreamSynchronize there -- "must be non nullptr" -- as soon
// as a replay or the stream mode ran on more than one host thread; round 5).
struct StreamPark { std::mutex mu; std::multimap<int, hipStream_t> idle; std::map<hipStream_t, std::vector<Deferred>> orphans; };
StreamPark &stream_park() { static StreamPark *p = new StreamPark(); return *p; }
hipStream_t take_parked_stream(int dev) {
    StreamPark &P = stream_park();
    hipStream_t st = nullptr;
    std::vector<std::pair<hipStream_t, std::vector<Deferred>>> drain;      // waited for and released OUTSIDE the lock: every ending thread's destructor needs it
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.idle.find(dev);
        if (it != P.idle.end()) {
            st = it->second;
            P.idle.erase(it);
            auto oi = P.orphans.find(st);
            if (oi != P.orphans.end()) { drain.emplace_back(st, std::move(oi->second)); P.orphans.erase(oi); }
        }
        // orphans nobody will ever adopt -- commands a thread left on the NULL stream (its stream creation had failed), or on a stream that is not
        // parked (the ending thread's aux stream was its main stream) -- would keep their pinned staging and device memory for the life of the
        // process: whoever comes by for a stream takes them along
        for (auto oi = P.orphans.begin(); oi != P.orphans.end();) {
            bool parked = false;
            for (auto &kv : P.idle) if (kv.second == oi->first) { parked = true; break; }
            if (!parked) { drain.emplace_back(oi->first, std::move(oi->second)); oi = P.orphans.erase(oi); } else ++oi;
        }
    }
    for (auto &d : drain) {      // what a stream's previous thread left in flight has long finished, as a rule: wait (here a HIP call is fine) and release
        (void)stream_wait(d.first);
        for (auto &x : d.second) { host_staging_release(x.h); (void)dev_free(x.d); }
    }
    return st;
}
ThreadStreams::~ThreadStreams() {
    if (main_thread) return;      // (the main thread's streams and whatever it left in flight go with the runtime's own teardown at process exit)
    StreamPark &P = stream_park();
    std::lock_guard<std::mutex> g(P.mu);
    for (auto &x : deferred) P.orphans[x.st].push_back(x);      // still in flight, possibly: released by the stream's next owner after its first wait
    deferred.clear();
    for (auto &kv : m) if (kv.second) P.idle.emplace(kv.first, kv.second);
    for (auto &kv : aux) if (kv.second) { bool own = true; for (auto &k2 : m) if (k2.second == kv.second) own = false; if (own) P.idle.emplace(kv.first, kv.second); }
}
}  // namespace
// the calling thread's second stream (created at first use): the native estimator runs a frame's marginalisation there, beside the next
// frame's association and upload on the thread's main stream
hipStream_t aux_stream() {
    ThreadStreams &mine = thread_streams();
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto it = mine.aux.find(dev);
    if (it != mine.aux.end()) return it->second;
    (void)util_stream();      // (sets main_thread)
    hipStream_t st = take_parked_stream(dev);
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = util_stream();
    mine.aux.emplace(dev, st);
    return st;
}
namespace { thread_local int g_stream_slot = 0; }
hipStream_t util_stream() {
    if (g_stream_slot == 1) { const int keep = g_stream_slot; g_stream_slot = 0; hipStream_t a = aux_stream(); g_stream_slot = keep; return a; }      // (aux_stream asks for the main one once, to learn whether this is the main thread)
    ThreadStreams &mine = thread_streams();
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto it = mine.m.find(dev);
    if (it != mine.m.end()) return it->second;
#if defined(__linux__)
    mine.main_thread = (long)syscall(SYS_gettid) == (long)getpid();
#else
    mine.main_thread = true;
#endif
    hipStream_t st = take_parked_stream(dev);
    if (!st && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;      // the default stream: slower, still correct
    mine.m.emplace(dev, st);
    return st;
}

int device_ready() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_err = "no HIP device visible: libtcv_hip has no CPU fallback";
        return TCV_ERR_NO_DEVICE;
    }
    return TCV_OK;
}
}  // namespace tcv

// ---- pinned host staging pool ----------------------------------------------------------------------------------------------
namespace tcv {
namespace {
struct HostBuf { void *p; size_t cap; bool busy; };
std::mutex g_host_mu;
std::vector<HostBuf> g_host_bufs;
enum { HOST_POOL_MAX = 24 };      // idle pinned buffers kept (a host thread that keeps two lock-step groups in flight holds four to six at a time; releasing one to the runtime costs a device-wide wait)
}  // namespace
static std::atomic<long long> g_host_allocs{0}, g_host_frees{0};
extern "C" long long tcv_debug_host_pool_allocs(void) { return g_host_allocs.load() * 1000000 + g_host_frees.load(); }
extern "C" long long tcv_debug_dev_pool_misses(void) { return tcv::dev_pool_misses(); }
void *host_staging_acquire(size_t bytes) {
    size_t cap = (size_t)1 << 20;
    while (cap < bytes) cap <<= 1;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        HostBuf *best = nullptr;
        for (auto &h : g_host_bufs) if (!h.busy && h.cap >= bytes && (!best || h.cap < best->cap)) best = &h;
        if (best) { best->busy = true; return best->p; }
    }
    void *p = nullptr;
    g_host_allocs++;
    if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host_bufs.push_back(HostBuf{p, cap, true});
    return p;
}
void host_staging_release(void *p) {
    if (!p) return;
    void *to_free = nullptr;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        size_t idle = 0;
        for (auto &h : g_host_bufs) if (!h.busy) idle++;
        for (size_t i = 0; i < g_host_bufs.size(); i++)
            if (g_host_bufs[i].p == p) {
                if (idle >= HOST_POOL_MAX) { to_free = p; g_host_bufs.erase(g_host_bufs.begin() + i); }
                else g_host_bufs[i].busy = false;
                break;
            }
    }
    if (to_free) { g_host_frees++; (void)hipHostFree(to_free); }
}
StagedTransfer::~StagedTransfer() { if (in_flight) (void)stream_wait(st); host_staging_release(host); (void)dev_free(dev); }
hipError_t StagedTransfer::wait() { const hipError_t e = stream_wait(st); if (e == hipSuccess) in_flight = false; return e; }
void StagedTransfer::park() { defer_release(host, dev, st); host = dev = nullptr; in_flight = false; }
int staged_download(void *dst, const void *d_src, size_t bytes, const char *what) {
    StagedTransfer dl(util_stream(), bytes);
    if (!dl.host) { set_error("hipHostMalloc (download staging) failed"); return TCV_ERR_HIP; }
    hipError_t e = bytes ? hipMemcpyAsync(dl.host, d_src, bytes, hipMemcpyDeviceToHost, dl.st) : hipSuccess;
    if (e == hipSuccess) { dl.issued(); e = dl.wait(); }
    if (e != hipSuccess) return hip_fail(e, what);
    std::memcpy(dst, dl.host, bytes);
    return TCV_OK;
}
int staged_upload(void *d_dst, const void *src, size_t bytes, const char *what) {
    StagedTransfer up(util_stream(), bytes);
    if (!up.host) { set_error("hipHostMalloc (upload staging) failed"); return TCV_ERR_HIP; }
    std::memcpy(up.host, src, bytes);
    up.issued();
    hipError_t e = hipMemcpyAsync(d_dst, up.host, bytes, hipMemcpyHostToDevice, up.st);
    const hipError_t ew = up.wait();
    if (e == hipSuccess) e = ew;
    return e == hipSuccess ? (int)TCV_OK : hip_fail(e, what);
}
}  // namespace tcv
using namespace tcv;

// =====================================================================================================
// library
// =====================================================================================================
extern "C" const char *tcv_version(void) { return "tcv-hip 0.1 (gfx950)"; }
extern "C" const char *tcv_last_error(void) { return g_err.c_str(); }
extern "C" int tcv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int tcv_device_memory_stats(unsigned long long *live_bytes, unsigned long long *cached_bytes, int *live_buffers) {
    tcv::dev_pool_stats(live_bytes, cached_bytes, live_buffers);
    return TCV_OK;
}
extern "C" int tcv_thread_stream_slot(int slot) {
    const int prev = g_stream_slot;
    g_stream_slot = slot == 1 ? 1 : 0;
    return prev;
}
extern "C" int tcv_set_device(int device) {
    if (int rc = device_ready()) return rc;
    HIPCHK(hipSetDevice(device));
    return TCV_OK;
}
