// Policy of the cooperative (small-batch) solve, as plain arithmetic (tcv_coop_policy.cpp: no HIP header, no HIP call): how many helper
// workgroups a window gets, and the per-device, per-XCD table that admits cooperative launches.  tests/dev/coop_policy_check.cpp pins both.
#pragma once
#include <cstddef>

namespace tcv {
enum { COOP_POLICY_MAX_H = 7 };      // = COOP_MAX_H of tcv_packed.h (checked where both are visible: tcv_batch_create.cpp)

// Helpers per window of a chain-layout batch of n windows whose largest window has `fmax` point / line factors, on a device of n_cu CUs.
// want: the request (tcv_set_cooperative, overridden by TCV_COOP_H): -1 automatic, 0 off, h >= 1 helpers; automatic: neither of the two
// was given -- only then does the policy for large batches apply, and a single helper become none.
int coop_helper_count(int n, size_t fmax, int n_cu, int want, bool automatic);

// what one cooperative launch in flight holds: CUs per XCD, their sum (0: no claim), and the XCD its first group lands on (SolveArgs::coop_rot)
struct CoopClaim { int xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0, rot = 0; };
// admission of a launch of `groups` groups of `wg` workgroups each on device `dev`: fills *c and returns true, or leaves the table and *c
// untouched and returns false (the caller then runs the same plan on one workgroup per window: same bits)
bool coop_admit(int dev, int n_cu, int groups, int wg, CoopClaim *c);
void coop_release(int dev, CoopClaim *c);      // gives the claim back (no-op without one); c->total = 0 afterwards
void coop_table(int dev, int out[8]);          // the CUs claimed per XCD on `dev`, for tests and diagnostics
}  // namespace tcv
