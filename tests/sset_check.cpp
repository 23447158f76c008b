// The host-only half of the sample-set analysis (csrc/pf_sset.h) as a program of its own: the block's layout, every rejection of
// pf_sample_set_analyze's arguments with its message, the cap arithmetic at the limits, and the packing into a buffer of exactly
// the planned size.  Built with the address and undefined-behaviour sanitizers by tests/test_sset_host.py; no HIP runtime call,
// no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "pf_sset.h"

using namespace pfsset;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

struct Case {
    std::vector<int32_t> set_ptr, center_ptr;
    pf_sset_opts_host o{1.0f, 1.5f, 0.5f};
    Case() {                                    // three sets of 1, 2 and 17 samples; center counts 1, 64, 2, then 6 each
        set_ptr = {0, 1, 3, 20};
        center_ptr = {0, 1, 65, 67};
        for (int s = 3; s < 20; ++s) center_ptr.push_back(center_ptr.back() + 6);
    }
    // sets of the given sizes, n centers in every sample
    Case(const std::vector<int>& sizes, int n) {
        set_ptr = {0};
        for (int S : sizes) set_ptr.push_back(set_ptr.back() + S);
        center_ptr.resize((size_t)set_ptr.back() + 1);
        for (size_t s = 0; s < center_ptr.size(); ++s) center_ptr[s] = (int32_t)(s * n);
    }
    SsetArgs args() const { return SsetArgs{(int)set_ptr.size() - 1, set_ptr.data(), center_ptr.data(), &o}; }
};

static bool ok(const SsetArgs& a, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says something
static void rejected(const SsetArgs& a, const char* needle) {
    std::string why;
    const bool r = ok(a, &why);
    if (r || why.find("pf_sample_set_analyze") == std::string::npos || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}

int main() {
    // ---- the layout: regions in order, nothing overlaps ----
    for (int P : {1, 2, 1000}) for (int S : {1, 33, 30000}) {
        const SsetLayout L(P, S);
        const size_t P1 = (size_t)P + 1;
        CHECK(L.set_ptr() == 0 && L.sim_ptr() == P1 && L.work_ptr() == 2 * P1 && L.center_ptr() == 3 * P1);
        CHECK(L.words() == 3 * P1 + (size_t)S + 1);
    }
    CHECK(tiles(1) == 1 && tiles(16) == 1 && tiles(17) == 2 && tiles(1024) == 64);
    CHECK(tile_pairs(1) == 1 && tile_pairs(17) == 3 && tile_pairs(33) == 6 && tile_pairs(1024) == 2080);
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args()));
    { Case d; d.o = {1e-3f, 0.f, 0.f}; CHECK(ok(d.args())); }                                   // tolerance 0, threshold 0
    { Case d; d.o.threshold = 1.f; CHECK(ok(d.args())); }
    { Case d({1024}, 64); CHECK(ok(d.args())); const SsetPlan pl = plan(d.args()); CHECK(pl.S == 1024 && pl.N == 65536 && pl.sim_floats == 1048576 && pl.work_items == 2080); }
    { Case d(std::vector<int>(64, 1024), 1); CHECK(ok(d.args())); CHECK(plan(d.args()).sim_floats == PF_SSET_MAX_SIM); }          // the cap itself
    // ---- every rejection ----
    { Case d(std::vector<int>(64, 1024), 1); d.set_ptr.push_back(d.set_ptr.back() + 1); d.center_ptr.push_back(d.center_ptr.back() + 1);
      rejected(d.args(), "67108865 floats (at most 67108864 per call"); }                       // one above
    { Case d({1025}, 1); rejected(d.args(), "set 0 has 1025 samples (1 to 1024 per set)"); }
    { Case d; d.set_ptr = {0, 1, 1, 20}; rejected(d.args(), "set 1 has 0 samples"); }
    { Case d; d.set_ptr = {0, 3, 1, 20}; rejected(d.args(), "set_ptr decreases at set 1"); }
    { Case d; d.set_ptr[0] = 1; rejected(d.args(), "set_ptr[0] must be 0"); }
    { Case d; d.center_ptr[0] = 1; rejected(d.args(), "center_ptr[0] must be 0"); }
    { Case d; d.center_ptr[2] = 66; rejected(d.args(), "sample 1 has 65 centers (1 to 64 per sample)"); }
    { Case d; d.center_ptr[1] = 0; rejected(d.args(), "sample 0 has 0 centers"); }
    { Case d; d.center_ptr[3] = 60; rejected(d.args(), "center_ptr decreases at sample 2"); }
    for (float bad : {0.f, -1.f, kNan, kInf}) { Case d; d.o.sigma = bad; rejected(d.args(), "sigma must be finite and > 0"); }
    for (float bad : {-0.5f, kNan, kInf}) { Case d; d.o.tolerance = bad; rejected(d.args(), "tolerance must be finite and >= 0"); }
    for (float bad : {-0.1f, 1.5f, kNan, kInf}) { Case d; d.o.threshold = bad; rejected(d.args(), "threshold must be in [0, 1]"); }
    { SsetArgs a = c.args(); a.P = 0; rejected(a, "0 sets"); }
    { SsetArgs a = c.args(); a.set_ptr = nullptr; rejected(a, "null"); }
    { SsetArgs a = c.args(); a.center_ptr = nullptr; rejected(a, "null"); }
    { SsetArgs a = c.args(); a.opts = nullptr; rejected(a, "null"); }
    { char msg[8]; Case d; d.set_ptr[0] = 1; const SsetArgs a = d.args(); CHECK(!validate(a, msg, sizeof msg) && msg[7] == 0); }  // a short message buffer
    // ---- the plan's scalars ----
    {
        Case d; d.o = {2.0f, 1.5f, 0.25f};
        const SsetPlan pl = plan(d.args());
        CHECK(pl.P == 3 && pl.S == 20 && pl.N == 67 + 17 * 6);
        CHECK(pl.sim_floats == 1 + 4 + 289 && pl.work_items == 1 + 1 + 3);
        CHECK(pl.inv_2s2 == 0.125f && pl.tol2 == 2.25f && pl.threshold == 0.25f);
    }
    // ---- packing: a buffer of exactly words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const SsetPlan pl = plan(c.args());
        const SsetLayout L(pl.P, pl.S);
        std::vector<uint32_t> st(L.words(), 0xdeadbeefu);
        pack(c.args(), st.data());
        const int32_t* q = (const int32_t*)st.data();
        for (int p = 0; p <= 3; ++p) CHECK(q[L.set_ptr() + p] == c.set_ptr[p]);
        for (int s = 0; s <= 20; ++s) CHECK(q[L.center_ptr() + s] == c.center_ptr[s]);
        const int32_t sim[4] = {0, 1, 5, 294}, work[4] = {0, 1, 2, 5};
        for (int p = 0; p <= 3; ++p) CHECK(q[L.sim_ptr() + p] == sim[p] && q[L.work_ptr() + p] == work[p]);
        for (uint32_t v : st) CHECK(v != 0xdeadbeefu);
    }
    {   // at the caps: 64 sets of 1024 samples, the last sim pointer is 2^26 and still an int32
        Case d(std::vector<int>(64, 1024), 1);
        const SsetLayout L(64, 65536);
        std::vector<uint32_t> st(L.words(), 0xdeadbeefu);
        pack(d.args(), st.data());
        const int32_t* q = (const int32_t*)st.data();
        CHECK(q[L.sim_ptr() + 64] == (int32_t)PF_SSET_MAX_SIM && q[L.work_ptr() + 64] == 64 * 2080 && q[L.center_ptr() + 65536] == 65536);
    }
    {   // one set of one sample with one center
        Case d({1}, 1);
        CHECK(ok(d.args()));
        const SsetLayout L(1, 1);
        std::vector<uint32_t> st(L.words(), 0xdeadbeefu);
        pack(d.args(), st.data());
        CHECK(L.words() == 8 && ((const int32_t*)st.data())[L.sim_ptr() + 1] == 1);
    }
    if (failures) { std::printf("sset_check: %d check(s) failed\n", failures); return 1; }
    std::printf("sset_check: all checks passed\n");
    return 0;
}
