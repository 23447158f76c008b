// The host-only half of the pharmacophore alignment (csrc/pf_align.h) as a program of its own: the block's layout, every rejection
// of pf_pharm_align's arguments with its message, the cap arithmetic at the limits, and the packing into a buffer of exactly the
// planned size; then the arithmetic of a pair (csrc/pf_align_core.h) run serially on the host: a rigid copy is found again, a
// mirror image is not, every rotation is proper.  Built with the address and undefined-behaviour sanitizers by
// tests/test_align_host.py; no HIP runtime call, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pf_align.h"
#include "pf_align_core.h"

using namespace pfalign;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

struct Case {
    std::vector<int32_t> q_ptr, l_ptr;
    pf_align_opts_host o{1.0f, 1.5f, 4, 1.0f};
    Case() : q_ptr{0, 1, 17, 20}, l_ptr{0, 32, 33, 35, 41} {}          // queries of 1, 16, 3 centers; entries of 32, 1, 2, 6
    Case(int Q, int nq, int L, int nl) {                                // Q queries of nq centers, L entries of nl
        q_ptr.resize((size_t)Q + 1); l_ptr.resize((size_t)L + 1);
        for (size_t s = 0; s < q_ptr.size(); ++s) q_ptr[s] = (int32_t)(s * nq);
        for (size_t s = 0; s < l_ptr.size(); ++s) l_ptr[s] = (int32_t)(s * nl);
    }
    AlignArgs args() const { return AlignArgs{(int)q_ptr.size() - 1, q_ptr.data(), (int)l_ptr.size() - 1, l_ptr.data(), &o}; }
};

static bool ok(const AlignArgs& a, std::string* why = nullptr) {
    char msg[256] = "";
    const bool r = validate(a, msg, sizeof msg);
    if (why) *why = msg;
    return r;
}
// a rejection names the function and says something
static void rejected(const AlignArgs& a, const char* needle) {
    std::string why;
    const bool r = ok(a, &why);
    if (r || why.find("pf_pharm_align") == std::string::npos || why.find(needle) == std::string::npos) {
        std::printf("FAILED: expected a rejection naming '%s', got %s '%s'\n", needle, r ? "acceptance" : "the message", why.c_str());
        ++failures;
    }
}

static float det3(const float* R) {
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

int main() {
    // ---- the layout: regions in order, nothing overlaps ----
    for (int Q : {1, 3, 4096}) for (int L : {1, 130, 100000}) {
        const AlignLayout lay(Q, L);
        CHECK(lay.q_ptr() == 0 && lay.l_ptr() == (size_t)Q + 1 && lay.words() == (size_t)Q + 1 + (size_t)L + 1);
    }
    // ---- what is accepted ----
    Case c;
    CHECK(ok(c.args()));
    { Case d; d.o = {1e-3f, 0.f, 0, 1e-6f}; CHECK(ok(d.args())); }                               // tolerance 0, no refinement
    { Case d; d.o.refine = 16; CHECK(ok(d.args())); }
    { Case d(4096, 16, 4096, 32); CHECK(ok(d.args())); const AlignPlan pl = plan(d.args());     // the pair cap itself
      CHECK(pl.pairs == PF_ALIGN_MAX_PAIRS && pl.Nq == 65536 && pl.Nl == 131072); }
    { Case d(1, 1, 1 << 24, 1); CHECK(ok(d.args())); CHECK(plan(d.args()).pairs == PF_ALIGN_MAX_PAIRS); }
    // ---- every rejection ----
    { Case d(4097, 1, 4096, 1); rejected(d.args(), "16781312 pairs (at most 16777216 per call"); }      // one row above
    { Case d(1, 1, (1 << 24) + 1, 1); rejected(d.args(), "16777217 pairs"); }
    { Case d(46341, 1, 46341, 1); rejected(d.args(), "2147488281 pairs"); }                     // the product needs 64 bits
    { Case d; d.q_ptr[0] = 1; rejected(d.args(), "q_ptr[0] must be 0"); }
    { Case d; d.l_ptr[0] = 2; rejected(d.args(), "l_ptr[0] must be 0"); }
    { Case d; d.q_ptr = {0, 1, 18, 20}; rejected(d.args(), "query 1 has 17 centers (1 to 16 per query)"); }
    { Case d; d.q_ptr = {0, 1, 1, 20}; rejected(d.args(), "query 1 has 0 centers"); }
    { Case d; d.q_ptr = {0, 5, 3, 20}; rejected(d.args(), "q_ptr decreases at query 1"); }
    { Case d; d.l_ptr = {0, 33, 34, 35, 41}; rejected(d.args(), "entry 0 has 33 centers (1 to 32 per entry)"); }
    { Case d; d.l_ptr = {0, 32, 32, 35, 41}; rejected(d.args(), "entry 1 has 0 centers"); }
    { Case d; d.l_ptr = {0, 32, 33, 30, 41}; rejected(d.args(), "l_ptr decreases at entry 2"); }
    for (float bad : {0.f, -1.f, kNan, kInf}) { Case d; d.o.sigma = bad; rejected(d.args(), "sigma must be finite and > 0"); }
    for (float bad : {-0.5f, kNan, kInf}) { Case d; d.o.tolerance = bad; rejected(d.args(), "tolerance must be finite and >= 0"); }
    for (int bad : {-1, 17, 1 << 30}) { Case d; d.o.refine = bad; rejected(d.args(), "refine must be in [0, 16]"); }
    for (float bad : {0.f, -1.f, kNan, kInf}) { Case d; d.o.min_area = bad; rejected(d.args(), "min_area must be finite and > 0"); }
    { AlignArgs a = c.args(); a.Q = 0; rejected(a, "0 queries"); }
    { AlignArgs a = c.args(); a.L = 0; rejected(a, "0 library entries"); }
    { AlignArgs a = c.args(); a.Q = -3; rejected(a, "-3 queries"); }
    { AlignArgs a = c.args(); a.q_ptr = nullptr; rejected(a, "null"); }
    { AlignArgs a = c.args(); a.l_ptr = nullptr; rejected(a, "null"); }
    { AlignArgs a = c.args(); a.opts = nullptr; rejected(a, "null"); }
    { char msg[8]; Case d; d.q_ptr[0] = 1; const AlignArgs a = d.args(); CHECK(!validate(a, msg, sizeof msg) && msg[7] == 0); }   // a short message buffer
    // ---- the plan's scalars ----
    {
        Case d; d.o = {2.0f, 1.5f, 7, 0.5f};
        const AlignPlan pl = plan(d.args());
        CHECK(pl.Q == 3 && pl.L == 4 && pl.Nq == 20 && pl.Nl == 41 && pl.pairs == 12 && pl.refine == 7);
        CHECK(pl.inv_2s2 == 0.125f && pl.tol2 == 2.25f && pl.seed_tol == 3.0f && pl.min_area == 0.5f);
    }
    // ---- packing: a buffer of exactly words() words (the sanitizer watches its ends), every value where the layout says ----
    {
        const AlignLayout lay(3, 4);
        std::vector<uint32_t> st(lay.words(), 0xdeadbeefu);
        pack(c.args(), st.data());
        const int32_t* q = (const int32_t*)st.data();
        for (int k = 0; k <= 3; ++k) CHECK(q[lay.q_ptr() + k] == c.q_ptr[k]);
        for (int k = 0; k <= 4; ++k) CHECK(q[lay.l_ptr() + k] == c.l_ptr[k]);
        for (uint32_t v : st) CHECK(v != 0xdeadbeefu);
    }
    {   // one query of one center against one entry of one center
        Case d(1, 1, 1, 1);
        CHECK(ok(d.args()));
        const AlignLayout lay(1, 1);
        std::vector<uint32_t> st(lay.words(), 0xdeadbeefu);
        pack(d.args(), st.data());
        CHECK(lay.words() == 4 && ((const int32_t*)st.data())[3] == 1);
    }
    // ---- a seed's key orders like (i, j, k, a, b, c) ----
    CHECK(align_key(0, 1, 2, 31, 30, 29) < align_key(0, 1, 3, 0, 1, 2) && align_key(1, 2, 3, 0, 1, 2) > align_key(0, 14, 15, 31, 30, 29));
    CHECK(align_key(13, 14, 15, 31, 30, 29) > 0 && align_key(2, 5, 9, 4, 1, 7) < align_key(2, 5, 9, 4, 2, 0));
    // ---- the arithmetic of a pair, serially on the host ----
    {
        // a chiral query: five centers of distinct types, not coplanar
        const float x[15] = {0.f, 0.f, 0.f,  3.f, 0.2f, 0.1f,  0.5f, 2.8f, -0.3f,  1.1f, 0.9f, 2.6f,  -1.7f, 1.4f, 1.2f};
        const int t[5] = {0, 1, 2, 3, 4};
        // the same under a proper rotation (about z by 90 degrees, then about x by 180) and a shift of tens of angstroms, permuted
        float y[15], m[15];
        int u[5], perm[5] = {3, 0, 4, 1, 2};
        for (int k = 0; k < 5; ++k) {
            const float* p = x + perm[k] * 3;
            y[k * 3] = -p[1] + 25.f; y[k * 3 + 1] = -p[0] - 31.f; y[k * 3 + 2] = -p[2] + 17.f;      // (x, y, z) -> (-y, -x, -z): det +1
            m[k * 3] = -x[k * 3]; m[k * 3 + 1] = x[k * 3 + 1]; m[k * 3 + 2] = x[k * 3 + 2];       // the mirror image
            u[k] = t[perm[k]];
        }
        unsigned mask[5];
        AlignResult r;
        int n = align_pair_serial(5, x, t, 5, y, u, mask, 0.5f, 2.25f, 3.0f, 1.0f, 4, r);
        CHECK(n == 10 && r.matched == 5 && r.sim >= 1.f - 1e-5f && std::fabs(det3(r.xf) - 1.f) < 1e-5f);
        for (int k = 0; k < 5; ++k) for (int e = 0; e < 3; ++e) {
            const float v = r.xf[e * 3] * y[k * 3] + r.xf[e * 3 + 1] * y[k * 3 + 1] + r.xf[e * 3 + 2] * y[k * 3 + 2] + r.xf[9 + e];
            CHECK(std::fabs(v - x[perm[k] * 3 + e]) < 1e-3f);
        }
        n = align_pair_serial(5, x, t, 5, m, t, mask, 0.5f, 2.25f, 3.0f, 1.0f, 4, r);
        CHECK(n == 10 && r.sim < 0.9f && r.sim > 0.1f && std::fabs(det3(r.xf) - 1.f) < 1e-5f);   // an improper rotation would give 1
        // two centers: no seed, the identity
        n = align_pair_serial(2, x, t, 5, y, u, mask, 0.5f, 2.25f, 3.0f, 1.0f, 4, r);
        CHECK(n == 0 && r.sim == 0.f && r.matched == 0 && r.xf[0] == 1.f && r.xf[4] == 1.f && r.xf[8] == 1.f && r.xf[1] == 0.f && r.xf[11] == 0.f);
        // an entry of collinear centers: every seed fails the area test
        float l[9] = {0.f, 0.f, 0.f, 1.5f, 0.f, 0.f, 3.f, 0.f, 0.f};
        n = align_pair_serial(5, x, t, 3, l, t, mask, 0.5f, 2.25f, 3.0f, 1.0f, 4, r);
        CHECK(n == 0 && r.sim == 0.f);
        // a degenerate solve (all zeros) still yields a proper rotation and no NaN
        float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, R[9];
        align_rotation(S, R);
        CHECK(std::fabs(det3(R) - 1.f) < 1e-6f);
    }
    if (failures) { std::printf("align_check: %d check(s) failed\n", failures); return 1; }
    std::printf("align_check: all checks passed\n");
    return 0;
}
