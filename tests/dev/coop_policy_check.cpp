// Host only, stand-alone: the cooperative mode's policy (tc-viml_amd/csrc/tcv_coop_policy.cpp) -- the helper count of a batch and the
// per-XCD admission table of cooperative launches -- pinned at the points where it decides.  No device, no library.  From the repository
// root (tests/test_coop_policy_cpu.py does the same into a temporary directory):
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/dev/coop_policy_check.cpp
//       tc-viml_amd/csrc/tcv_coop_policy.cpp -o /tmp/coop_policy_check && /tmp/coop_policy_check      (one line)
#include <cstdio>
#include <cstring>

#include "../../tc-viml_amd/csrc/tcv_coop_policy.h"

using namespace tcv;

static int g_failed = 0;
#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); g_failed++; }          \
    } while (0)

struct Table {
    int v[8];
    explicit Table(int dev) { coop_table(dev, v); }
    bool is(int x0, int x1, int x2, int x3, int x4, int x5, int x6, int x7) const {
        const int w[8] = {x0, x1, x2, x3, x4, x5, x6, x7};
        return std::memcmp(v, w, sizeof v) == 0;
    }
    bool all(int x) const { return is(x, x, x, x, x, x, x, x); }
    bool operator==(const Table &o) const { return std::memcmp(v, o.v, sizeof v) == 0; }
};

static void admission() {
    const int n_cu = 256;      // 32 CUs per XCD
    {   // five launches of one group of eight workgroups: each lands on the XCD with the fewest claims, ties to the lowest index
        CoopClaim c[5];
        for (int k = 0; k < 5; k++) {
            CHECK(coop_admit(0, n_cu, 1, 8, &c[k]));
            CHECK(c[k].rot == k && c[k].total == 8 && c[k].xcd[k] == 8);
        }
        CHECK(Table(0).is(8, 8, 8, 8, 8, 0, 0, 0));
        for (int k = 0; k < 5; k++) coop_release(0, &c[k]);
        CHECK(Table(0).all(0));
    }
    {   // eight groups of eight workgroups: 8 CUs on every XCD per launch, so four fit and the fifth does not
        CoopClaim c[5];
        for (int k = 0; k < 4; k++) { CHECK(coop_admit(0, n_cu, 8, 8, &c[k])); CHECK(c[k].total == 64 && c[k].rot == 0); }
        CHECK(Table(0).all(32));
        const Table before(0);
        CoopClaim untouched;
        std::memcpy(&untouched, &c[4], sizeof untouched);
        CHECK(!coop_admit(0, n_cu, 8, 8, &c[4]));
        CHECK(Table(0) == before);                                      // a refusal leaves the table as it was,
        CHECK(std::memcmp(&untouched, &c[4], sizeof untouched) == 0);    // and the claim
        {   // two devices: device 1 knows nothing of device 0's claims
            CoopClaim d;
            CHECK(Table(1).all(0));
            CHECK(coop_admit(1, n_cu, 8, 8, &d));
            CHECK(Table(1).all(8) && Table(0).all(32));
            coop_release(1, &d);
            CHECK(Table(1).all(0) && Table(0).all(32));
        }
        coop_release(0, &c[1]);
        CHECK(c[1].total == 0 && Table(0).all(24));
        CHECK(coop_admit(0, n_cu, 8, 8, &c[4]));
        CHECK(Table(0).all(32));
        coop_release(0, &c[1]);      // (no claim: no-op)
        CHECK(Table(0).all(32));
        for (int k = 0; k < 5; k++) coop_release(0, &c[k]);
        CHECK(Table(0).all(0));
    }
    {   // nine groups of four workgroups onto a table whose minimum is at XCD 3: the ninth group wraps onto the first group's XCD
        CoopClaim pre, c;
        CHECK(coop_admit(0, n_cu, 3, 1, &pre));
        CHECK(Table(0).is(1, 1, 1, 0, 0, 0, 0, 0));
        CHECK(coop_admit(0, n_cu, 9, 4, &c));
        CHECK(c.rot == 3 && c.total == 36);
        for (int x = 0; x < 8; x++) CHECK(c.xcd[x] == (x == 3 ? 8 : 4));
        CHECK(Table(0).is(5, 5, 5, 8, 4, 4, 4, 4));
        coop_release(0, &pre); coop_release(0, &c);
        CHECK(Table(0).all(0));
    }
    {   // n_cu = 8: one CU per XCD
        CoopClaim c;
        CHECK(coop_admit(0, 8, 1, 1, &c));
        CHECK(c.total == 1 && c.rot == 0);
        coop_release(0, &c);
        CHECK(!coop_admit(0, 8, 1, 2, &c));
        CHECK(c.total == 0 && Table(0).all(0));
    }
}

static void helper_count() {
    const int n_cu = 256;
    // automatic, no override: one helper per ~96 factors of the largest window, at least two, as many as the XCDs hold
    CHECK(coop_helper_count(1, 95, n_cu, -1, true) == 0);
    CHECK(coop_helper_count(1, 96, n_cu, -1, true) == 2);
    CHECK(coop_helper_count(1, 600, n_cu, -1, true) == 7);
    CHECK(coop_helper_count(8, 600, n_cu, -1, true) == 7);
    CHECK(coop_helper_count(9, 600, n_cu, -1, true) == 7);      // two groups per XCD x 8 = 16 <= 32
    CHECK(coop_helper_count(64, 600, n_cu, -1, true) == 2);     // from 24 windows on: half the chip, three quarters for two helpers
    CHECK(coop_helper_count(65, 600, n_cu, -1, true) == 0);
    // an explicit request is honoured, a single helper too; the automatic path turns one helper into none
    CHECK(coop_helper_count(1, 600, n_cu, 1, false) == 1);
    CHECK(coop_helper_count(20, 600, 64, 7, false) == 1);       // (8 CUs per XCD, three groups on each: 3 x (1 + 1) <= 8)
    CHECK(coop_helper_count(20, 600, 64, -1, true) == 0);
    CHECK(coop_helper_count(1, 600, n_cu, 0, false) == 0);
    // an explicit 7 with 40 windows: cut to what ceil(n / 8) x (1 + h) <= n_cu / 8 allows
    const int h = coop_helper_count(40, 600, n_cu, 7, false);
    CHECK(h == 5 && 5 * (1 + h) <= n_cu / 8 && 5 * (2 + h) > n_cu / 8);
    CHECK(coop_helper_count(1, 600, n_cu, 100, false) == COOP_POLICY_MAX_H);
}

int main() {
    admission();
    helper_count();
    if (g_failed) { std::printf("coop_policy_check: %d check(s) FAILED\n", g_failed); return 1; }
    std::printf("coop_policy_check: ok\n");
    return 0;
}
