// The host-only half of type guidance (csrc/pf_types.h) as a program of its own: the block's layout, every rejection of
// pf_guide_types_next's arguments, and the packing into a buffer of exactly the planned size.  Built with the address and
// undefined-behaviour sanitizers by tests/test_types_host.py; no HIP runtime call, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pf_types.h"

using namespace pftypes;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Case {
    int B = 3, nt = 6;
    std::vector<int32_t> pharm_ptr, ptr, center, type;
    std::vector<float> p, r, w;
    float scale = 1.f, clip = 0.f, sharp = 4.f, unmatched = 0.f;
    int32_t comp = 0;
    Case() {
        pharm_ptr = {0, 3, 4, 9};               // 3, 1 and 5 centers
        ptr = {0, 2, 2, 5};
        center = {-1, 2, 0, -1, 4};
        type = {0, 5, 3, 1, 2};
        for (int j = 0; j < 5; ++j) { for (int c = 0; c < 3; ++c) p.push_back(0.5f * j - c); r.push_back(j % 2 ? 0.f : 2.5f); w.push_back(1.f + j); }
    }
    TypesArgs args() const {
        return TypesArgs{ptr.data(), center.data(), type.data(), p.data(), r.data(), w.data(), scale, clip, sharp, comp, unmatched};
    }
};

static bool ok(const TypesArgs& a, const Case& c, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, c.B, c.pharm_ptr.data(), c.nt, msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says something
static void rejected(const TypesArgs& a, const Case& c, const char* needle) {
    std::string why;
    const bool r = ok(a, c, &why);
    if (r || why.find("pf_guide_types_next") == std::string::npos || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- the layout: regions in order, nothing overlaps ----
    for (int B : {0, 1, 5}) for (int n : {0, 1, 70, 256 * 5}) {
        const TypesLayout tl(B, n);
        const size_t n1 = n > 1 ? n : 1, B1 = (size_t)B + 1;
        CHECK(tl.ptr() == 0 && tl.center() == B1 && tl.type() == tl.center() + n1 && tl.p() == tl.type() + n1);
        CHECK(tl.r() == tl.p() + 3 * n1 && tl.w() == tl.r() + n1 && tl.words() == tl.w() + n1);
    }
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args(), c));
    { TypesArgs a = c.args(); a.ptr = nullptr; a.center = nullptr; a.type = nullptr; a.p = nullptr; a.r = nullptr; a.w = nullptr; CHECK(ok(a, c)); }
    { TypesArgs a = c.args(); a.feat_scale = 0.f; a.feat_clip = 0.f; a.type_sharpness = 0.f; a.unmatched = 0.f; CHECK(ok(a, c)); }
    { TypesArgs a = c.args(); a.comp_types = 1; a.unmatched = 1.5f; a.feat_clip = 2.f; CHECK(ok(a, c)); }
    { Case d; d.ptr = {0, 0, 0, 0}; TypesArgs a = d.args(); a.center = nullptr; a.type = nullptr; a.p = nullptr; a.r = nullptr; a.w = nullptr; CHECK(ok(a, d)); }
    { Case d; d.ptr = {0, 256, 256, 256}; d.center.assign(256, -1); d.type.assign(256, 5); d.p.assign(256 * 3, 1.f); d.r.assign(256, 0.f);
      d.w.assign(256, 0.f); CHECK(ok(d.args(), d)); }
    { Case d; d.type[0] = 5; d.center[1] = 2; CHECK(ok(d.args(), d)); }                      // the last type, the last center
    // ---- every rejection ----
    for (float bad : {-1.f, nan, inf}) {
        { TypesArgs a = c.args(); a.feat_scale = bad; rejected(a, c, "feat_scale"); }
        { TypesArgs a = c.args(); a.feat_clip = bad; rejected(a, c, "feat_clip"); }
        { TypesArgs a = c.args(); a.type_sharpness = bad; rejected(a, c, "type_sharpness"); }
        { TypesArgs a = c.args(); a.unmatched = bad; rejected(a, c, "unmatched"); }
        { Case d; d.r[3] = bad; rejected(d.args(), d, "type restraint 3: the radius"); }
        { Case d; d.w[4] = bad; rejected(d.args(), d, "type restraint 4: the weight"); }
    }
    { TypesArgs a = c.args(); a.comp_types = 2; rejected(a, c, "comp_types"); }
    { Case d; d.p[4] = nan; rejected(d.args(), d, "type restraint 1 has a non-finite point"); }
    { Case d; d.p[14] = inf; rejected(d.args(), d, "type restraint 4 has a non-finite point"); }
    { Case d; d.type[2] = 6; rejected(d.args(), d, "type restraint 2 has type 6"); }
    { Case d; d.type[0] = -1; rejected(d.args(), d, "type restraint 0 has type -1"); }
    { Case d; d.center[1] = 3; rejected(d.args(), d, "names center 3 of graph 0, which has 3"); }
    { Case d; d.center[4] = 5; rejected(d.args(), d, "names center 5 of graph 2, which has 5"); }
    { Case d; d.center[0] = -2; rejected(d.args(), d, "names center -2"); }
    { Case d; d.ptr = {0, 2, 3, 5}; d.center[2] = 1; rejected(d.args(), d, "names center 1 of graph 1, which has 1"); }
    { Case d; d.ptr = {1, 2, 2, 5}; rejected(d.args(), d, "ptr[0]"); }
    { Case d; d.ptr = {0, 3, 2, 5}; rejected(d.args(), d, "decreases at graph 1"); }
    { Case d; d.ptr = {0, 257, 257, 257}; d.center.assign(257, -1); d.type.assign(257, 0); d.p.assign(257 * 3, 0.f); d.r.assign(257, 0.f);
      d.w.assign(257, 0.f); rejected(d.args(), d, "at most 256"); }
    { TypesArgs a = c.args(); a.center = nullptr; rejected(a, c, "null type restraint array"); }
    { TypesArgs a = c.args(); a.type = nullptr; rejected(a, c, "null type restraint array"); }
    { TypesArgs a = c.args(); a.p = nullptr; rejected(a, c, "null type restraint array"); }
    { TypesArgs a = c.args(); a.r = nullptr; rejected(a, c, "null type restraint array"); }
    { TypesArgs a = c.args(); a.w = nullptr; rejected(a, c, "null type restraint array"); }
    { char msg[64]; CHECK(!validate(c.args(), c.B, c.pharm_ptr.data(), 17, msg, sizeof msg)); }
    { char msg[64]; CHECK(!validate(c.args(), c.B, nullptr, 6, msg, sizeof msg)); }
    // ---- packing: a buffer of exactly words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const TypesLayout tl(c.B, n_restraints(c.args(), c.B));
        std::vector<uint32_t> st(tl.words(), 0xdeadbeefu);
        pack(c.args(), c.B, st.data());
        const float* f = (const float*)st.data(); const int32_t* q = (const int32_t*)st.data();
        for (int g = 0; g <= c.B; ++g) CHECK(q[tl.ptr() + g] == c.ptr[g]);
        for (int j = 0; j < 5; ++j) {
            CHECK(q[tl.center() + j] == c.center[j] && q[tl.type() + j] == c.type[j]);
            for (int k = 0; k < 3; ++k) CHECK(f[tl.p() + 3 * j + k] == c.p[3 * j + k]);
            CHECK(f[tl.r() + j] == c.r[j] && f[tl.w() + j] == c.w[j]);
        }
    }
    {   // no restraint array: no restraint in any graph, a block of zeros
        TypesArgs a = c.args(); a.ptr = nullptr;
        CHECK(n_restraints(a, c.B) == 0);
        const TypesLayout tl(c.B, 0);
        std::vector<uint32_t> st(tl.words(), 0xdeadbeefu);
        pack(a, c.B, st.data());
        for (uint32_t v : st) CHECK(v == 0u);
    }
    {   // the smallest batch: no graph
        Case d; d.B = 0; d.pharm_ptr = {0}; d.ptr = {0}; d.center.clear(); d.type.clear(); d.p.clear(); d.r.clear(); d.w.clear();
        CHECK(ok(d.args(), d));
        const TypesLayout tl(0, 0);
        std::vector<uint32_t> st(tl.words(), 0xdeadbeefu);
        pack(d.args(), 0, st.data());
        CHECK(tl.words() == 8);
    }
    if (failures) { std::printf("types_check: %d check(s) failed\n", failures); return 1; }
    std::printf("types_check: all checks passed\n");
    return 0;
}
