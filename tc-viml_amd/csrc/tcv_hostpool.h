// Host-side plumbing that every batch-level call shares (tcv_hostpool.cpp): the thread budget, the persistent worker threads and the
// free list of the plans' int-pool blocks.  Host code only: no device translation unit needs it.
#pragma once
#include <cstddef>
#include <functional>

namespace tcv {
// Host threads a batch-level operation may start: min(want, cores the process is GRANTED / batch-level operations running right now).
// The grant is the cgroup CPU quota (cpu.max) or the affinity mask, not the machine's thread count: four callers packing 512 windows each on
// sixteen threads under a 16-core quota used to run 64 threads into the scheduler's throttling.
struct HostOp { HostOp(); ~HostOp(); int threads(int want) const; };
int host_threads(int want);      // the same share for code that runs inside somebody's HostOp (does not count as an operation of its own)
// fn(t) for t in [0, nth): index claiming by the calling thread and by persistent worker threads (created once); returns
// when all have finished.  nth <= 1: plain call.
void parallel_run(int nth, const std::function<void(int)> &fn);
// items 0 .. n - 1 claimed ONE AT A TIME by up to nth threads (the caller among them): fn(item, slot), slot < nth unique per thread.  A
// worker that wakes up late finds fewer items instead of a fixed share nobody else may touch (a strided split of 64 windows over 8 threads
// waited a whole share -- 0.36 ms -- for the last two workers).
void parallel_items(int n, int nth, const std::function<void(int, int)> &fn);
void async_run(std::function<void()> fn);      // fn() on a worker thread, some time later; nobody waits (here and now if the process has no worker)
// Int pools of the plans (~170 KB per window) come from a process-wide free list of power-of-two blocks: a malloc of that size is a fresh
// mmap whose pages fault in on first touch (~100 us per plan, as much as building it); a live estimator makes and drops one per frame.
void *plan_block_alloc(size_t bytes);
void plan_block_free(void *p, size_t bytes);
}  // namespace tcv
