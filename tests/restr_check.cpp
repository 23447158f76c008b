// The host-only half of a guided run's restraints (csrc/pf_restr.h) as a program of its own: the block's layout, every acceptance
// and rejection of pf_sample_begin_guided's restraint arguments, the packing into a buffer of exactly the planned size, and the
// layouts of the two workspaces a guided step writes.  Built with the address and undefined-behaviour sanitizers by
// tests/test_restr_host.py; no HIP runtime call, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pf_restr.h"

using namespace pfrestr;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Case {
    int B = 3;
    std::vector<int32_t> pharm_ptr, ptr, kind, center;
    std::vector<float> p, r, w;
    float scale = 1.5f, clip = 0.5f;
    Case() {
        pharm_ptr = {0, 3, 4, 9};               // 3, 1 and 5 centers
        ptr = {0, 2, 2, 5};                     // the graph in the middle has no restraint
        kind = {0, 1, 1, 0, 1};
        center = {-1, 2, 0, -1, 4};
        for (int j = 0; j < 5; ++j) { for (int c = 0; c < 3; ++c) p.push_back(0.5f * j - c); r.push_back(j % 2 ? 0.f : 2.5f); w.push_back(1.f + j); }
    }
    void fill(int n) { kind.assign(n, 1); center.assign(n, -1); p.assign((size_t)n * 3, 1.f); r.assign(n, 0.f); w.assign(n, 0.f); }
    RestrArgs args() const { return RestrArgs{ptr.data(), kind.data(), center.data(), p.data(), r.data(), w.data(), scale, clip}; }
};

static bool ok(const RestrArgs& a, const Case& c, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, c.B, c.pharm_ptr.data(), msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says what today's message says
static void rejected(const RestrArgs& a, const Case& c, const char* needle) {
    std::string why;
    const bool r = ok(a, c, &why);
    if (r || why.find("pf_sample_begin_guided: ") != 0 || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- the layout: regions in order, nothing overlaps; both users' names over the two integer columns ----
    for (int B : {0, 1, 5}) for (int n : {0, 1, 70, 256 * 5}) {
        const RestrLayout rl(B, n);
        const size_t n1 = n > 1 ? n : 1, B1 = (size_t)B + 1;
        CHECK(rl.ptr() == 0 && rl.kind() == B1 && rl.center() == rl.kind() + n1 && rl.p() == rl.center() + n1);
        CHECK(rl.r() == rl.p() + 3 * n1 && rl.w() == rl.r() + n1 && rl.words() == rl.w() + n1);
        const BlockLayout bl(B, n);
        CHECK(bl.col_a() == rl.kind() && bl.col_b() == rl.center() && bl.words() == rl.words());
    }
    // ---- the workspaces: regions in order, nothing overlaps ----
    for (int B : {0, 1, 5}) for (int Nf : {0, 1, 23}) for (int nh : {1, 6, 16}) {
        const size_t nf1 = Nf > 1 ? Nf : 1, b = (size_t)B, h = (size_t)nh;
        const GuideWork gw(Nf, nh, B);
        CHECK(gw.g0() == 0 && gw.jx() == gw.g0() + 3 * nf1 && gw.grad() == gw.jx() + 3 * nf1 && gw.shift() == gw.grad() + 3 * nf1);
        CHECK(gw.zero() == gw.shift() + 3 * nf1 && gw.energy() == gw.zero() + nf1 * h && gw.D() == gw.energy() + b && gw.words() == gw.D() + 3 * b);
        const TypeWork tw(Nf, nh, B);
        CHECK(tw.g0_h() == 0 && tw.gs_h() == nf1 * h && tw.j_h() == 2 * nf1 * h && tw.grad_h() == 3 * nf1 * h && tw.shift_h() == 4 * nf1 * h);
        CHECK(tw.E_type() == 5 * nf1 * h && tw.words() == tw.E_type() + b);
    }
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args(), c));
    { RestrArgs a = c.args(); a.guide_scale = 0.f; a.guide_clip = 0.f; CHECK(ok(a, c)); }
    { Case d; d.ptr = {0, 0, 0, 0}; RestrArgs a = d.args(); a.kind = nullptr; a.center = nullptr; a.p = nullptr; a.r = nullptr; a.w = nullptr; CHECK(ok(a, d)); }
    { Case d; d.ptr = {0, 256, 256, 256}; d.fill(256); CHECK(ok(d.args(), d)); }            // 256 restraints in one graph
    { Case d; d.kind[0] = 1; d.center[1] = 2; d.center[4] = 4; d.center[2] = -1; CHECK(ok(d.args(), d)); }     // the last center, center -1
    { Case d; d.r[0] = 0.f; d.w[0] = 0.f; CHECK(ok(d.args(), d)); }
    // ---- every rejection, by the needle of its message ----
    { RestrArgs a = c.args(); a.ptr = nullptr; rejected(a, c, "null restr_ptr"); }
    for (float bad : {-1.f, nan, inf}) {
        { RestrArgs a = c.args(); a.guide_scale = bad; rejected(a, c, "guide_scale must be finite and >= 0"); }
        { RestrArgs a = c.args(); a.guide_clip = bad; rejected(a, c, "guide_clip must be finite and >= 0 (0: no clip)"); }
        { Case d; d.r[3] = bad; rejected(d.args(), d, ": restraint 3: the radius must be finite and >= 0"); }
        { Case d; d.w[4] = bad; rejected(d.args(), d, ": restraint 4: the weight must be finite and >= 0"); }
    }
    { Case d; d.p[4] = nan; rejected(d.args(), d, ": restraint 1 has a non-finite point"); }
    { Case d; d.p[14] = inf; rejected(d.args(), d, ": restraint 4 has a non-finite point"); }
    { Case d; d.p[0] = -inf; rejected(d.args(), d, ": restraint 0 has a non-finite point"); }
    { Case d; d.kind[2] = 2; rejected(d.args(), d, ": restraint 2 has kind 2 (0 attract, 1 repel)"); }
    { Case d; d.kind[0] = -1; rejected(d.args(), d, ": restraint 0 has kind -1 (0 attract, 1 repel)"); }
    { Case d; d.center[1] = 3; rejected(d.args(), d, ": restraint 1 names center 3 of graph 0, which has 3 (-1: every center)"); }
    { Case d; d.center[4] = 5; rejected(d.args(), d, ": restraint 4 names center 5 of graph 2, which has 5 (-1: every center)"); }
    { Case d; d.center[0] = -2; rejected(d.args(), d, ": restraint 0 names center -2 of graph 0"); }
    { Case d; d.ptr = {0, 2, 3, 5}; d.center[2] = 1; rejected(d.args(), d, ": restraint 2 names center 1 of graph 1, which has 1"); }
    { Case d; d.ptr = {1, 2, 2, 5}; rejected(d.args(), d, ": restr_ptr[0] must be 0"); }
    { Case d; d.ptr = {0, 3, 2, 5}; rejected(d.args(), d, ": restr_ptr decreases at graph 1"); }
    { Case d; d.ptr = {0, 257, 257, 257}; d.fill(257); rejected(d.args(), d, ": graph 0 has 257 restraints (at most 256 per graph)"); }
    { RestrArgs a = c.args(); a.kind = nullptr; rejected(a, c, ": null restraint array"); }
    { RestrArgs a = c.args(); a.center = nullptr; rejected(a, c, ": null restraint array"); }
    { RestrArgs a = c.args(); a.p = nullptr; rejected(a, c, ": null restraint array"); }
    { RestrArgs a = c.args(); a.r = nullptr; rejected(a, c, ": null restraint array"); }
    { RestrArgs a = c.args(); a.w = nullptr; rejected(a, c, ": null restraint array"); }
    // a row with two faults: the kind is reported before the other columns
    { Case d; d.kind[1] = 7; d.center[1] = 9; d.r[1] = nan; rejected(d.args(), d, ": restraint 1 has kind 7"); }
    // ---- packing: a buffer of exactly words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const RestrLayout rl(c.B, n_restraints(c.args(), c.B));
        std::vector<uint32_t> st(rl.words(), 0xdeadbeefu);
        pack(c.args(), c.B, st.data());
        const float* f = (const float*)st.data(); const int32_t* q = (const int32_t*)st.data();
        for (int g = 0; g <= c.B; ++g) CHECK(q[rl.ptr() + g] == c.ptr[g]);
        for (int j = 0; j < 5; ++j) {
            CHECK(q[rl.kind() + j] == c.kind[j] && q[rl.center() + j] == c.center[j]);
            for (int k = 0; k < 3; ++k) CHECK(f[rl.p() + 3 * j + k] == c.p[3 * j + k]);
            CHECK(f[rl.r() + j] == c.r[j] && f[rl.w() + j] == c.w[j]);
        }
    }
    {   // no restraint in any graph, no arrays: ptr and a row of zeros
        Case d; d.ptr = {0, 0, 0, 0};
        RestrArgs a = d.args(); a.kind = nullptr; a.center = nullptr; a.p = nullptr; a.r = nullptr; a.w = nullptr;
        CHECK(n_restraints(a, d.B) == 0);
        const RestrLayout rl(d.B, 0);
        std::vector<uint32_t> st(rl.words(), 0xdeadbeefu);
        pack(a, d.B, st.data());
        for (uint32_t v : st) CHECK(v == 0u);
    }
    {   // 256 restraints in every graph of five
        Case d; d.B = 5; d.pharm_ptr = {0, 3, 11, 16, 17, 23}; d.ptr = {0, 256, 512, 768, 1024, 1280}; d.fill(1280);
        CHECK(ok(d.args(), d));
        const RestrLayout rl(d.B, 1280);
        std::vector<uint32_t> st(rl.words(), 0xdeadbeefu);
        pack(d.args(), d.B, st.data());
        CHECK(((const int32_t*)st.data())[rl.ptr() + 5] == 1280 && ((const int32_t*)st.data())[rl.center() + 1279] == -1);
    }
    {   // the smallest batch: no graph
        Case d; d.B = 0; d.pharm_ptr = {0}; d.ptr = {0}; d.fill(0);
        CHECK(ok(d.args(), d));
        const RestrLayout rl(0, 0);
        std::vector<uint32_t> st(rl.words(), 0xdeadbeefu);
        pack(d.args(), 0, st.data());
        CHECK(rl.words() == 8);
        for (uint32_t v : st) CHECK(v == 0u);
    }
    if (failures) { std::printf("restr_check: %d check(s) failed\n", failures); return 1; }
    std::printf("restr_check: all checks passed\n");
    return 0;
}
