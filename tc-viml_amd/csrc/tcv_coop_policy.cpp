// The cooperative mode's policy (tcv_coop_policy.h): the helper count of a batch and the admission table of cooperative launches.  Pure
// arithmetic behind a mutex -- no HIP header, no HIP call, nothing of tcv_batch.
#include "tcv_coop_policy.h"

#include <algorithm>
#include <mutex>

namespace tcv {

// Cooperative mode (tcv_packed.h COOP_*): a chain-layout batch that leaves most of the chip idle gives every window 1 + H workgroups.
// H: one helper per ~96 point / line factors of the largest window (`fmax` of them), as many as the CUs allow.  TCV_COOP_H overrides (0: off).
int coop_helper_count(int n, size_t fmax, int n_cu, int want, bool automatic) {
    if (want < 0) want = fmax >= 96 ? std::min<int>(COOP_POLICY_MAX_H, std::max<int>(2, (int)((fmax + 95) / 96))) : 0;
    want = std::min(want, (int)COOP_POLICY_MAX_H);
    while (want > 0 && (long long)((n + 7) / 8) * (1 + want) > n_cu / 8) want--;      // the groups of a launch are dealt round-robin to the XCDs: per XCD ceil(n / 8) groups on n_cu / 8 CUs
    // A large batch seldom has the device to itself -- a lock-step replay drives it from two host threads, and a launch that fills the chip with
    // helpers makes the other thread's launch queue behind it (64 streams: 10.8 K windows/s with seven helpers per window against 12.1 K with
    // two; 128 streams: 15.5 K with three against 17.7 K with two; profiles/r05_replay_coop_helpers.txt).  From 24 windows on a launch takes
    // half the chip -- three quarters if that is what two helpers per window need; TCV_COOP_H / tcv_set_cooperative still decide otherwise.
    if (n >= 24 && automatic) {
        int w2 = want;
        while (w2 > 0 && (long long)n * (1 + w2) > n_cu / 2) w2--;
        if (w2 < 2 && want >= 2 && (long long)n * 3 <= (long long)n_cu * 3 / 4) w2 = 2;
        want = std::min(want, w2);
    }
    if (want == 1 && automatic) want = 0;      // a single helper is not worth the hand-offs
    return want;
}

// CUs claimed by cooperative launches in flight, per device AND per XCD: a cooperative kernel spins on its partners, so all cooperative
// grids in flight together must be resident (two half-resident cooperative kernels could wait for each other's CUs until their
// timeouts).  The members of a group share an XCD -- workgroup b of a launch is dispatched to XCD b % 8 and solve_kernel makes the
// members of group g the workgroups with b % 8 == (g + rot) % 8 -- so the budget that counts is the XCD's (n_cu / 8 CUs), not the
// chip's: five one-window batches of eight workgroups each, all starting at XCD 0, would pass a chip-wide count (40 of 256) and
// sit half-resident on that XCD's 32 CUs.  A launch therefore (1) rotates its groups so that its first group lands on the XCD with the
// fewest claimed CUs (CoopClaim::rot) and (2) is admitted only if every XCD keeps its claims within its CUs.
static std::mutex g_coop_mu;
static int g_coop_claimed[64][8];

bool coop_admit(int dev, int n_cu, int groups, int wg, CoopClaim *c) {
    std::lock_guard<std::mutex> g(g_coop_mu);
    int *cl = g_coop_claimed[dev & 63];
    const int per_xcd = std::max(1, n_cu / 8);
    int rot = 0;
    for (int x = 1; x < 8; x++) if (cl[x] < cl[rot]) rot = x;
    int need[8];
    for (int x = 0; x < 8; x++) need[x] = 0;
    for (int q = 0; q < 8; q++) need[(q + rot) & 7] = wg * ((groups + 7 - q) / 8);      // groups g = q, q + 8, ... land on XCD (q + rot) % 8
    for (int x = 0; x < 8; x++) if (cl[x] + need[x] > per_xcd) return false;
    int total = 0;
    for (int x = 0; x < 8; x++) { cl[x] += need[x]; c->xcd[x] = need[x]; total += need[x]; }
    c->total = total; c->rot = rot;
    return true;
}
void coop_release(int dev, CoopClaim *c) {
    if (c->total > 0) {
        std::lock_guard<std::mutex> g(g_coop_mu);
        for (int x = 0; x < 8; x++) g_coop_claimed[dev & 63][x] -= c->xcd[x];
        c->total = 0;
    }
}
void coop_table(int dev, int out[8]) {
    std::lock_guard<std::mutex> g(g_coop_mu);
    for (int x = 0; x < 8; x++) out[x] = g_coop_claimed[dev & 63][x];
}

}  // namespace tcv
