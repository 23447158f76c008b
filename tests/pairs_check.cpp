// The host-only half of pair guidance (csrc/pf_pairs.h) as a program of its own: the block's layout, every rejection of
// pf_guide_pairs_next's arguments, and the packing into a buffer of exactly the planned size.  Built with the address and
// undefined-behaviour sanitizers by tests/test_pairs_host.py; no HIP runtime call, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pf_pairs.h"

using namespace pfpairs;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

struct Case {
    int B = 3;
    std::vector<int32_t> pharm_ptr, ptr, i, j;
    std::vector<float> lo, hi, w;
    Case() {
        pharm_ptr = {0, 3, 4, 9};               // 3, 1 and 5 centers
        ptr = {0, 2, 3, 6};
        i = {-1, 0, -1, 1, 4, -1};              // every form: (*, *), (i, j), (*, *) on the single center, (i, j), (i, *), (*, j)
        j = {-1, 2, -1, 3, -1, 0};
        lo = {3.f, 0.f, 4.f, 5.f, 0.f, 2.5f};
        hi = {kInf, 6.f, kInf, 7.f, 0.f, 2.5f};
        w = {1.f, 2.f, 1.f, 0.f, 0.5f, 3.f};
    }
    PairsArgs args() const { return PairsArgs{ptr.data(), i.data(), j.data(), lo.data(), hi.data(), w.data()}; }
};

static bool ok(const PairsArgs& a, const Case& c, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, c.B, c.pharm_ptr.data(), msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says something
static void rejected(const PairsArgs& a, const Case& c, const char* needle) {
    std::string why;
    const bool r = ok(a, c, &why);
    if (r || why.find("pf_guide_pairs_next") == std::string::npos || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}
static Case full(int n) {                       // n (*, *) restraints on graph 0
    Case d; d.ptr = {0, n, n, n}; d.i.assign(n, -1); d.j.assign(n, -1); d.lo.assign(n, 1.f); d.hi.assign(n, kInf); d.w.assign(n, 0.f);
    return d;
}

int main() {
    // ---- the layout: regions in order, nothing overlaps ----
    for (int B : {0, 1, 5}) for (int n : {0, 1, 70, 256 * 5}) {
        const PairsLayout pl(B, n);
        const size_t n1 = n > 1 ? n : 1, B1 = (size_t)B + 1;
        CHECK(pl.ptr() == 0 && pl.i() == B1 && pl.j() == pl.i() + n1 && pl.lo() == pl.j() + n1);
        CHECK(pl.hi() == pl.lo() + n1 && pl.w() == pl.hi() + n1 && pl.words() == pl.w() + n1);
    }
    {
        const PairWork pw(23, 5);
        CHECK(pw.g_pair() == 0 && pw.E_pair() == 69 && pw.words() == 74);
        CHECK(PairWork(0, 0).words() == 3);
    }
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args(), c));                     // hi = +inf, lo == hi, lo == 0, w == 0, the last center, a wildcard on either side
    { PairsArgs a = c.args(); a.ptr = nullptr; a.i = nullptr; a.j = nullptr; a.lo = nullptr; a.hi = nullptr; a.w = nullptr; CHECK(ok(a, c)); }
    { Case d; d.ptr = {0, 0, 0, 0}; PairsArgs a = d.args(); a.i = nullptr; a.j = nullptr; a.lo = nullptr; a.hi = nullptr; a.w = nullptr; CHECK(ok(a, d)); }   // n = 0
    { Case d = full(256); CHECK(ok(d.args(), d)); }
    { Case d; d.i[0] = -1; d.j[0] = 2; d.i[4] = 4; d.j[4] = 3; CHECK(ok(d.args(), d)); }
    // ---- every rejection ----
    { Case d; d.j[1] = 0; rejected(d.args(), d, "pair restraint 1 names center 0 twice"); }                   // i == j
    { Case d; d.i[1] = 3; rejected(d.args(), d, "names center 3 of graph 0, which has 3"); }
    { Case d; d.j[3] = 5; rejected(d.args(), d, "names center 5 of graph 2, which has 5"); }
    { Case d; d.i[2] = 1; rejected(d.args(), d, "names center 1 of graph 1, which has 1"); }
    { Case d; d.j[0] = -2; rejected(d.args(), d, "names center -2"); }
    { Case d; d.lo[3] = 8.f; rejected(d.args(), d, "pair restraint 3: hi must be >= lo"); }                    // lo > hi
    { Case d; d.hi[0] = -kInf; rejected(d.args(), d, "pair restraint 0: hi must be >= lo"); }                  // hi = -inf
    { Case d; d.hi[1] = kNan; rejected(d.args(), d, "pair restraint 1: hi must be >= lo"); }
    { Case d; d.lo[1] = kNan; rejected(d.args(), d, "pair restraint 1: lo must be finite"); }
    { Case d; d.lo[0] = kInf; rejected(d.args(), d, "pair restraint 0: lo must be finite"); }
    { Case d; d.lo[1] = -1.f; rejected(d.args(), d, "pair restraint 1: lo must be finite and >= 0"); }
    for (float bad : {-1.f, kNan, kInf}) { Case d; d.w[5] = bad; rejected(d.args(), d, "pair restraint 5: the weight"); }
    { Case d; d.ptr = {1, 2, 3, 6}; rejected(d.args(), d, "ptr[0]"); }
    { Case d; d.ptr = {0, 3, 2, 6}; rejected(d.args(), d, "decreases at graph 1"); }                          // a non-monotone ptr
    { Case d = full(257); rejected(d.args(), d, "at most 256"); }
    { Case d; d.pharm_ptr = {0, 3, 4, 69}; rejected(d.args(), d, "graph 2 has 65 centers"); }
    { Case d; d.pharm_ptr = {0, 3, 4, 69}; d.ptr = {0, 2, 3, 3}; CHECK(ok(d.args(), d)); }                    // (no pair restraint there: accepted)
    { PairsArgs a = c.args(); a.i = nullptr; rejected(a, c, "null pair restraint array"); }
    { PairsArgs a = c.args(); a.j = nullptr; rejected(a, c, "null pair restraint array"); }
    { PairsArgs a = c.args(); a.lo = nullptr; rejected(a, c, "null pair restraint array"); }
    { PairsArgs a = c.args(); a.hi = nullptr; rejected(a, c, "null pair restraint array"); }
    { PairsArgs a = c.args(); a.w = nullptr; rejected(a, c, "null pair restraint array"); }
    { char msg[64]; CHECK(!validate(c.args(), c.B, nullptr, msg, sizeof msg)); }
    { char msg[8]; Case d; d.j[1] = 0; CHECK(!validate(d.args(), d.B, d.pharm_ptr.data(), msg, sizeof msg) && msg[7] == 0); }     // a short message buffer
    // ---- packing: a buffer of exactly words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const PairsLayout pl(c.B, n_restraints(c.args(), c.B));
        std::vector<uint32_t> st(pl.words(), 0xdeadbeefu);
        pack(c.args(), c.B, st.data());
        const float* f = (const float*)st.data(); const int32_t* q = (const int32_t*)st.data();
        for (int g = 0; g <= c.B; ++g) CHECK(q[pl.ptr() + g] == c.ptr[g]);
        for (int k = 0; k < 6; ++k) {
            CHECK(q[pl.i() + k] == c.i[k] && q[pl.j() + k] == c.j[k]);
            CHECK(f[pl.lo() + k] == c.lo[k] && f[pl.hi() + k] == c.hi[k] && f[pl.w() + k] == c.w[k]);
        }
    }
    {   // the cap: 256 on one graph
        Case d = full(256);
        const PairsLayout pl(d.B, 256);
        std::vector<uint32_t> st(pl.words(), 0xdeadbeefu);
        pack(d.args(), d.B, st.data());
        CHECK(((const int32_t*)st.data())[pl.i() + 255] == -1 && std::isinf(((const float*)st.data())[pl.hi() + 255]));
    }
    {   // no ptr: no restraint in any graph, a block of zeros
        PairsArgs a = c.args(); a.ptr = nullptr;
        CHECK(n_restraints(a, c.B) == 0);
        const PairsLayout pl(c.B, 0);
        std::vector<uint32_t> st(pl.words(), 0xdeadbeefu);
        pack(a, c.B, st.data());
        for (uint32_t v : st) CHECK(v == 0u);
    }
    {   // n = 0 with a ptr: the same block, the column pointers are never read
        Case d; d.ptr = {0, 0, 0, 0};
        PairsArgs a = d.args(); a.i = nullptr; a.j = nullptr; a.lo = nullptr; a.hi = nullptr; a.w = nullptr;
        const PairsLayout pl(d.B, 0);
        std::vector<uint32_t> st(pl.words(), 0xdeadbeefu);
        pack(a, d.B, st.data());
        for (uint32_t v : st) CHECK(v == 0u);
    }
    {   // the smallest batch: no graph
        Case d; d.B = 0; d.pharm_ptr = {0}; d.ptr = {0}; d.i.clear(); d.j.clear(); d.lo.clear(); d.hi.clear(); d.w.clear();
        CHECK(ok(d.args(), d));
        const PairsLayout pl(0, 0);
        std::vector<uint32_t> st(pl.words(), 0xdeadbeefu);
        pack(d.args(), 0, st.data());
        CHECK(pl.words() == 6);
    }
    if (failures) { std::printf("pairs_check: %d check(s) failed\n", failures); return 1; }
    std::printf("pairs_check: all checks passed\n");
    return 0;
}
