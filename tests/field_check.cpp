// The host-only half of the pocket field (csrc/pf_field.h) as a program of its own: the block's layout, every rejection of
// pf_guide_field_next's arguments, and the packing into a buffer of exactly the planned size.  Built with the address and
// undefined-behaviour sanitizers by tests/test_field_host.py; no HIP runtime call, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pf_field.h"

using namespace pffield;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Case {
    int B = 3, Np = 10, nt = 6;
    std::vector<float> atom_r, ph_x, dist;
    std::vector<int32_t> ph_ptr, ph_type, match;
    float w_clash = 1.f, w_comp = 0.25f, kappa = 4.f, sharp = 4.f;
    Case() {
        atom_r.assign(Np, 2.f); atom_r[3] = 0.f;
        ph_ptr = {0, 0, 4, 5};
        for (int j = 0; j < 5; ++j) { ph_type.push_back(j % nt); for (int c = 0; c < 3; ++c) ph_x.push_back(0.5f * j - c); }
        match.assign(nt * nt, 0);
        for (int t = 0; t < nt; ++t) match[t * nt + (t + 1) % nt] = 1;
        dist = {7.f, 4.f, 4.f, 5.f, 5.f, 5.f};
    }
    FieldArgs args() const {
        return FieldArgs{atom_r.data(), w_clash, ph_ptr.data(), ph_x.data(), ph_type.data(), match.data(), dist.data(), w_comp, kappa, sharp};
    }
};

static bool ok(const FieldArgs& a, const Case& c, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, c.B, c.Np, c.nt, msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says something
static void rejected(const FieldArgs& a, const Case& c, const char* needle) {
    std::string why;
    const bool r = ok(a, c, &why);
    if (r || why.find("pf_guide_field_next") == std::string::npos || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- the layout: regions in order, nothing overlaps, the feature rows are 16-byte aligned ----
    for (int Np : {0, 1, 10, 601}) for (int B : {0, 1, 5}) for (int n : {0, 1, 70, 4096 * 5}) for (int nt : {1, 6, 16}) {
        const FieldLayout fl(Np, B, n, nt);
        const size_t n1 = n > 1 ? n : 1, Np1 = Np > 1 ? Np : 1;
        CHECK(fl.ph_xt() == 0 && fl.atom_r() == 4 * n1 && fl.ph_ptr() == fl.atom_r() + Np1);
        CHECK(fl.match() == fl.ph_ptr() + (size_t)B + 1 && fl.dist() == fl.match() + (size_t)nt * nt);
        CHECK(fl.upload_words() == fl.dist() + (size_t)nt && fl.e3() == fl.upload_words() && fl.words() == fl.e3() + (size_t)B * 3);
    }
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args(), c));
    { FieldArgs a = c.args(); a.atom_r = nullptr; CHECK(ok(a, c)); }                        // no clash term
    { FieldArgs a = c.args(); a.ph_ptr = nullptr; a.ph_x = nullptr; a.ph_type = nullptr; a.match = nullptr; a.dist = nullptr; CHECK(ok(a, c)); }
    { FieldArgs a = c.args(); a.atom_r = nullptr; a.ph_ptr = nullptr; a.w_clash = 0.f; a.w_comp = 0.f; CHECK(ok(a, c)); }
    { FieldArgs a = c.args(); a.w_clash = 0.f; a.w_comp = 0.f; a.type_sharpness = 0.f; CHECK(ok(a, c)); }
    { Case d; d.ph_ptr = {0, 0, 0, 0}; FieldArgs a = d.args(); a.ph_x = nullptr; a.ph_type = nullptr; CHECK(ok(a, d)); }   // no feature at all
    { Case d; d.ph_ptr = {0, 4096, 4096, 4096}; d.ph_type.assign(4096, 2); d.ph_x.assign(4096 * 3, 1.f); CHECK(ok(d.args(), d)); }
    // ---- every rejection ----
    for (float bad : {-1.f, nan, inf}) {
        { FieldArgs a = c.args(); a.w_clash = bad; rejected(a, c, "w_clash"); }
        { FieldArgs a = c.args(); a.w_comp = bad; rejected(a, c, "w_comp"); }
        { FieldArgs a = c.args(); a.kappa = bad; rejected(a, c, "kappa"); }
        { FieldArgs a = c.args(); a.type_sharpness = bad; rejected(a, c, "type_sharpness"); }
        { Case d; d.atom_r[7] = bad; rejected(d.args(), d, "atom 7"); }
        { Case d; d.dist[2] = bad; rejected(d.args(), d, "distance of type 2"); }
    }
    { FieldArgs a = c.args(); a.kappa = 0.f; rejected(a, c, "kappa"); }
    { Case d; d.ph_x[4] = nan; rejected(d.args(), d, "feature 1"); }
    { Case d; d.ph_type[2] = 6; rejected(d.args(), d, "feature 2"); }
    { Case d; d.ph_type[0] = -1; rejected(d.args(), d, "feature 0"); }
    { Case d; d.ph_ptr = {1, 1, 4, 5}; rejected(d.args(), d, "ph_ptr[0]"); }
    { Case d; d.ph_ptr = {0, 3, 2, 5}; rejected(d.args(), d, "decreases at graph 1"); }
    { Case d; d.ph_ptr = {0, 4097, 4097, 4097}; d.ph_type.assign(4097, 0); d.ph_x.assign(4097 * 3, 0.f); rejected(d.args(), d, "4096"); }
    { Case d; d.match[7] = 2; rejected(d.args(), d, "match[1][1]"); }
    { FieldArgs a = c.args(); a.match = nullptr; rejected(a, c, "match table"); }
    { FieldArgs a = c.args(); a.dist = nullptr; rejected(a, c, "match table"); }
    { FieldArgs a = c.args(); a.ph_x = nullptr; rejected(a, c, "null receptor feature array"); }
    { FieldArgs a = c.args(); a.ph_type = nullptr; rejected(a, c, "null receptor feature array"); }
    { char msg[64]; CHECK(!validate(c.args(), c.B, c.Np, 17, msg, sizeof msg)); }
    // ---- packing: a buffer of exactly upload_words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const FieldLayout fl(c.Np, c.B, n_features(c.args(), c.B), c.nt);
        std::vector<uint32_t> st(fl.upload_words(), 0xdeadbeefu);
        pack(c.args(), c.B, c.Np, c.nt, st.data());
        const float* f = (const float*)st.data(); const int32_t* w = (const int32_t*)st.data();
        for (int j = 0; j < 5; ++j) {
            for (int k = 0; k < 3; ++k) CHECK(f[fl.ph_xt() + 4 * j + k] == c.ph_x[3 * j + k]);
            CHECK(w[fl.ph_xt() + 4 * j + 3] == c.ph_type[j]);
        }
        for (int i = 0; i < c.Np; ++i) CHECK(f[fl.atom_r() + i] == c.atom_r[i]);
        for (int g = 0; g <= c.B; ++g) CHECK(w[fl.ph_ptr() + g] == c.ph_ptr[g]);
        for (int i = 0; i < c.nt * c.nt; ++i) CHECK(w[fl.match() + i] == c.match[i]);
        for (int t = 0; t < c.nt; ++t) CHECK(f[fl.dist() + t] == c.dist[t]);
    }
    {   // absent terms: radii of zero, no feature in any graph
        FieldArgs a = c.args(); a.atom_r = nullptr; a.ph_ptr = nullptr;
        CHECK(n_features(a, c.B) == 0);
        const FieldLayout fl(c.Np, c.B, 0, c.nt);
        std::vector<uint32_t> st(fl.upload_words(), 0xdeadbeefu);
        pack(a, c.B, c.Np, c.nt, st.data());
        for (uint32_t v : st) CHECK(v == 0u);
    }
    {   // the smallest batch: no atom, no graph
        Case d; d.B = 0; d.Np = 0; d.atom_r.clear(); d.ph_ptr = {0}; d.ph_x.clear(); d.ph_type.clear();
        CHECK(ok(d.args(), d));
        const FieldLayout fl(0, 0, 0, d.nt);
        std::vector<uint32_t> st(fl.upload_words(), 0xdeadbeefu);
        pack(d.args(), 0, 0, d.nt, st.data());
        CHECK(fl.words() == fl.upload_words());
    }
    if (failures) { std::printf("field_check: %d check(s) failed\n", failures); return 1; }
    std::printf("field_check: all checks passed\n");
    return 0;
}
