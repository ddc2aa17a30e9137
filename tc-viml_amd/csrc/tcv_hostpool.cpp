// Host thread budget, persistent worker threads and the block pool of the plans' int pools (tcv_hostpool.h): shared by the packer, the
// batch-level entry points, the marginalisation's host side, the line association and the native estimator.
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "tcv_hostpool.h"

namespace tcv {

// ---- host thread budget (HostOp)
static int host_core_grant_probe() {
    int g = (int)std::thread::hardware_concurrency();
    if (g <= 0) g = 1;
#if defined(__linux__)
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) g = std::min(g, c); }
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {      // cgroup v2: "<quota> <period>" or "max <period>"
        char q[64]; long long per = 0;
        if (fscanf(f, "%63s %lld", q, &per) == 2 && per > 0 && strcmp(q, "max") != 0) { const long long quota = atoll(q); if (quota > 0) g = std::min<long long>(g, std::max<long long>(1, (quota + per - 1) / per)); }
        fclose(f);
    } else if (FILE *f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {      // cgroup v1
        long long quota = -1, per = 0;
        if (fscanf(f1, "%lld", &quota) != 1) quota = -1;
        fclose(f1);
        if (FILE *f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f2, "%lld", &per) != 1) per = 0; fclose(f2); }
        if (quota > 0 && per > 0) g = std::min<long long>(g, std::max<long long>(1, (quota + per - 1) / per));
    }
#endif
    if (const char *e = getenv("TCV_HOST_THREADS")) { const int v = atoi(e); if (v > 0) g = v; }
    return std::max(1, g);
}
static int host_core_grant() {
    static const int grant = host_core_grant_probe();      // (once: several host threads ask at the same time)
    return grant;
}
static std::atomic<int> g_host_ops{0};
HostOp::HostOp() { g_host_ops.fetch_add(1, std::memory_order_relaxed); }
HostOp::~HostOp() { g_host_ops.fetch_sub(1, std::memory_order_relaxed); }
int host_threads(int want) {
    const int active = std::max(1, g_host_ops.load(std::memory_order_relaxed));
    return std::max(1, std::min(want, std::max(1, host_core_grant() / active)));
}
int HostOp::threads(int want) const { return host_threads(want); }

// ---- persistent worker threads (parallel_run) --------------------------------------------------------------------------------
// A batch-level call has three or four short parallel sections (plans, data, marginalisation problems, copies): 16 std::thread
// creations and joins per section were ~2 ms of a 512-window tcv_batch_create.  The workers are created once (up to the core grant
// minus the caller), sleep on a condition variable and claim task indices of the posted calls; the CALLER claims indices too, so a call
// makes progress whatever the workers are busy with, and returns when every index has finished.  The pool object is never destroyed
// (the detached workers may outlive static destruction).  A worker without work sleeps at once: polling for the next section first was
// measured at 8 / 64 / 128 replay streams and gave the same windows/s for 15 - 40 % more CPU time.
namespace {
struct ParCall {
    const std::function<void(int)> *fn;
    std::function<void(int)> own;      // async_run: the call owns its function (nobody waits for it)
    int n;
    std::atomic<int> next{0}, done{0};
    std::mutex mu;
    std::condition_variable cv;
};
struct WorkerPool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<ParCall>> q;
    int nworkers = 0;
    std::atomic<int> sleepers{0};         // workers inside cv.wait: a post with nobody asleep skips the futex
};
WorkerPool &worker_pool() { static WorkerPool *P = new WorkerPool(); return *P; }
void run_call(ParCall &c) {
    for (;;) {
        const int t = c.next.fetch_add(1, std::memory_order_relaxed);
        if (t >= c.n) return;
        (*c.fn)(t);
        if (c.done.fetch_add(1, std::memory_order_acq_rel) + 1 == c.n) { std::lock_guard<std::mutex> g(c.mu); c.cv.notify_all(); }
    }
}
void worker_main() {
    WorkerPool &P = worker_pool();
    for (;;) {
        std::shared_ptr<ParCall> c;
        {
            std::unique_lock<std::mutex> g(P.mu);
            for (;;) {
                while (!P.q.empty() && P.q.front()->next.load(std::memory_order_relaxed) >= P.q.front()->n) P.q.pop_front();      // fully claimed
                if (!P.q.empty()) { c = P.q.front(); break; }
                P.sleepers.fetch_add(1, std::memory_order_relaxed);
                P.cv.wait(g);
                P.sleepers.fetch_sub(1, std::memory_order_relaxed);
            }
        }
        run_call(*c);
    }
}
void wait_call(ParCall &c) {
    std::unique_lock<std::mutex> g(c.mu);
    c.cv.wait(g, [&] { return c.done.load(std::memory_order_acquire) >= c.n; });
}
}  // namespace
void parallel_run(int nth, const std::function<void(int)> &fn) {
    if (nth <= 1) { fn(0); return; }
    WorkerPool &P = worker_pool();
    auto c = std::make_shared<ParCall>();
    c->fn = &fn; c->n = nth;
    bool wake;
    {
        std::lock_guard<std::mutex> g(P.mu);
        const int want = std::min(31, std::max(1, host_core_grant() - 1));
        while (P.nworkers < std::min(want, nth - 1)) { std::thread(worker_main).detach(); P.nworkers++; }
        P.q.push_back(c);
        wake = P.sleepers.load(std::memory_order_relaxed) > 0;
    }
    if (wake) P.cv.notify_all();
    run_call(*c);
    wait_call(*c);
}

void parallel_items(int n, int nth, const std::function<void(int, int)> &fn) {
    if (n <= 0) return;
    nth = std::min(nth, n);
    if (nth <= 1) { for (int i = 0; i < n; i++) fn(i, 0); return; }
    std::atomic<int> next{0};
    parallel_run(nth, [&](int t) { for (;;) { const int i = next.fetch_add(1, std::memory_order_relaxed); if (i >= n) return; fn(i, t); } });
}

// fire and forget on the worker pool (the retired problems of a lock-step frame are destroyed this way: 0.3 ms of the caller's frame
// at 64 windows).  Without workers -- a one-core grant -- the function runs here.
void async_run(std::function<void()> fn) {
    WorkerPool &P = worker_pool();
    bool have_worker;
    {
        std::lock_guard<std::mutex> g(P.mu);
        if (P.nworkers == 0 && host_core_grant() > 1) { std::thread(worker_main).detach(); P.nworkers++; }
        have_worker = P.nworkers > 0;
    }
    if (!have_worker) { fn(); return; }
    auto c = std::make_shared<ParCall>();
    auto sp = std::make_shared<std::function<void()>>(std::move(fn));
    c->own = [sp](int) { (*sp)(); };
    c->fn = &c->own; c->n = 1;
    { std::lock_guard<std::mutex> g(P.mu); P.q.push_back(c); }
    P.cv.notify_one();
}

// ---- blocks of the plans' int pools (PlanAlloc, tcv_host.h): power-of-two size classes from 16 KB, a bounded free list per class
namespace {
struct BlockPool { std::mutex mu; std::vector<void *> idle[12]; };      // 16 KB .. 32 MB
BlockPool &block_pool() { static BlockPool *p = new BlockPool(); return *p; }
inline int block_class(size_t bytes, size_t &cap) { int c = 0; cap = (size_t)16 << 10; while (cap < bytes) { cap <<= 1; c++; } return c; }
}  // namespace
void *plan_block_alloc(size_t bytes) {
    if (bytes < ((size_t)16 << 10)) return ::operator new(bytes);
    size_t cap;
    const int c = block_class(bytes, cap);
    if (c < 12) {
        BlockPool &P = block_pool();
        std::lock_guard<std::mutex> g(P.mu);
        if (!P.idle[c].empty()) { void *p = P.idle[c].back(); P.idle[c].pop_back(); return p; }
    }
    return ::operator new(cap);
}
void plan_block_free(void *p, size_t bytes) {
    if (!p) return;
    if (bytes < ((size_t)16 << 10)) { ::operator delete(p); return; }
    size_t cap;
    const int c = block_class(bytes, cap);
    if (c < 12) {
        BlockPool &P = block_pool();
        std::lock_guard<std::mutex> g(P.mu);
        if (P.idle[c].size() < (size_t)(c <= 5 ? 192 : 8)) { P.idle[c].push_back(p); return; }      // (<= 512 KB: the plans of a lock-step frame; larger blocks: a handful)
    }
    ::operator delete(p);
}

}  // namespace tcv
