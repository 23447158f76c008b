// The point-restraint block of a guided run, host only -- no HIP runtime call, no handle (tests/restr_check.cpp runs all of it without a
// GPU).  Two users share it: the spatial restraints of pf_sample_begin_guided (below: their arguments, checks and packing) and the type
// restraints of pf_guide_types_next (pf_types.h).  The layouts of the two workspaces a guided step writes are named here too.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define PF_RESTR_MAX_PER_GRAPH 256      // restraints of one user per graph

namespace pfrestr {

// The block (the device allocation and its staging buffer), in 32-bit words, n1 = max(n, 1), all of it uploaded:
//   ptr [B + 1]  col_a [n1]  col_b [n1]  p [n1][3]  r [n1]  w [n1]
// The two integer columns are the center (a local index, -1: every center of the graph) and the user's tag, in the order that
// user's kernel was written for: each user names them over this struct
struct BlockLayout {
    size_t B1, n1;
    BlockLayout(int B, int n) : B1((size_t)B + 1), n1((size_t)(n > 1 ? n : 1)) {}
    size_t ptr() const { return 0; }            size_t col_a() const { return B1; }             size_t col_b() const { return B1 + n1; }
    size_t p() const { return B1 + 2 * n1; }    size_t r() const { return B1 + 5 * n1; }        size_t w() const { return B1 + 6 * n1; }
    size_t words() const { return B1 + 7 * n1; }
};

// The caller's host arrays in the block's column order; what its messages carry: the function, a row's noun, the ptr argument's name
struct Block { const int32_t *ptr, *col_a, *col_b; const float *p, *r, *w; };
struct Words { const char *who, *noun, *ptr; };

#define PF_RESTR_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)
inline bool bad_scalar(float v) { return !(v >= 0.f) || !std::isfinite(v); }

// The checks both users share, against the bound batch (B graphs, pharm_ptr [B + 1] its centers); b.ptr is not NULL.  center: b.col_a or
// b.col_b.  tag_ok(j, msg, msg_len): the user's check of row j's tag, run first in the row.  false: msg holds what was wrong
template <class TagOk>
inline bool validate_block(const Block& b, const int32_t* center, int B, const int32_t* pharm_ptr, const Words& t, TagOk tag_ok, char* msg, size_t msg_len) {
    if (b.ptr[0] != 0) PF_RESTR_BAD("%s: %s[0] must be 0", t.who, t.ptr);
    for (int g = 0; g < B; ++g) {
        const int n = b.ptr[g + 1] - b.ptr[g];
        if (n < 0) PF_RESTR_BAD("%s: %s decreases at graph %d", t.who, t.ptr, g);
        if (n > PF_RESTR_MAX_PER_GRAPH) PF_RESTR_BAD("%s: graph %d has %d %ss (at most %d per graph)", t.who, g, n, t.noun, PF_RESTR_MAX_PER_GRAPH);
    }
    if (b.ptr[B] > 0 && (!b.col_a || !b.col_b || !b.p || !b.r || !b.w)) PF_RESTR_BAD("%s: null %s array", t.who, t.noun);
    for (int g = 0; g < B; ++g) {
        const int nf_g = pharm_ptr[g + 1] - pharm_ptr[g];
        for (int j = b.ptr[g]; j < b.ptr[g + 1]; ++j) {
            if (!tag_ok(j, msg, msg_len)) return false;
            if (center[j] < -1 || center[j] >= nf_g)
                PF_RESTR_BAD("%s: %s %d names center %d of graph %d, which has %d (-1: every center)", t.who, t.noun, j, (int)center[j], g, nf_g);
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(b.p[(size_t)j * 3 + c])) PF_RESTR_BAD("%s: %s %d has a non-finite point", t.who, t.noun, j);
            if (bad_scalar(b.r[j])) PF_RESTR_BAD("%s: %s %d: the radius must be finite and >= 0", t.who, t.noun, j);
            if (bad_scalar(b.w[j])) PF_RESTR_BAD("%s: %s %d: the weight must be finite and >= 0", t.who, t.noun, j);
        }
    }
    return true;
}

// Validated arrays into the staging buffer, in the block's layout (words() words are written).  No ptr: no restraint in any graph
inline void pack_block(const Block& b, int B, uint32_t* st) {
    const int n = b.ptr ? b.ptr[B] : 0;
    const BlockLayout bl(B, n);
    std::memset(st, 0, bl.words() * 4);
    if (!b.ptr) return;
    std::memcpy(st + bl.ptr(), b.ptr, bl.B1 * 4);
    const void* col[5] = {b.col_a, b.col_b, b.p, b.r, b.w};
    const size_t at[6] = {bl.col_a(), bl.col_b(), bl.p(), bl.r(), bl.w(), bl.words()};       // (a column is as wide as the next one is far)
    for (int k = 0; n > 0 && k < 5; ++k) std::memcpy(st + at[k], col[k], (at[k + 1] - at[k]) / bl.n1 * (size_t)n * 4);
}

// ---- the spatial restraints of pf_sample_begin_guided: the columns are kind (0 attract, 1 repel), center ----
struct RestrArgs {
    const int32_t *ptr, *kind, *center; const float *p, *r, *w; float guide_scale, guide_clip;
    Block block() const { return Block{ptr, kind, center, p, r, w}; }
};
struct RestrLayout : BlockLayout { using BlockLayout::BlockLayout; size_t kind() const { return col_a(); } size_t center() const { return col_b(); } };
// Every check of pf_sample_begin_guided's restraint arguments against the bound batch
inline bool validate(const RestrArgs& a, int B, const int32_t* pharm_ptr, char* msg, size_t msg_len) {
    const Words t{"pf_sample_begin_guided", "restraint", "restr_ptr"};
    if (!a.ptr) PF_RESTR_BAD("%s: null restr_ptr", t.who);
    if (bad_scalar(a.guide_scale)) PF_RESTR_BAD("%s: guide_scale must be finite and >= 0", t.who);
    if (bad_scalar(a.guide_clip)) PF_RESTR_BAD("%s: guide_clip must be finite and >= 0 (0: no clip)", t.who);
    return validate_block(a.block(), a.center, B, pharm_ptr, t, [&](int j, char* msg, size_t msg_len) {
        if (a.kind[j] != 0 && a.kind[j] != 1) PF_RESTR_BAD("%s: restraint %d has kind %d (0 attract, 1 repel)", t.who, j, (int)a.kind[j]);
        return true;
    }, msg, msg_len);
}
inline int n_restraints(const RestrArgs& a, int B) { return a.ptr[B]; }
inline void pack(const RestrArgs& a, int B, uint32_t* st) { pack_block(a.block(), B, st); }
#undef PF_RESTR_BAD

// ---- what a guided step leaves, in 32-bit words (nf1 = max(Nf, 1), nh = pharm_nf) ----
// d_guide:  g0 [nf1][3]  jx = J(g0) [nf1][3]  grad [nf1][3]  shift [nf1][3]  zero [nf1][nh] (a step's g_eps_h without a feature gradient; cleared at begin)  energy [B]  D [B][3]
struct GuideWork {
    size_t nf1, nh, B;
    GuideWork(int Nf, int nh_, int B_) : nf1((size_t)(Nf > 1 ? Nf : 1)), nh((size_t)nh_), B((size_t)B_) {}
    size_t g0() const { return 0; }             size_t jx() const { return nf1 * 3; }           size_t grad() const { return nf1 * 6; }
    size_t shift() const { return nf1 * 9; }    size_t zero() const { return nf1 * 12; }        size_t energy() const { return nf1 * (12 + nh); }
    size_t D() const { return energy() + B; }   size_t words() const { return D() + B * 3; }
};
// d_tguide (type guidance):  g0_h  gs_h = (phi_h / phi_x) g0_h  j_h  grad_h  shift_h [nf1][nh] each  E_type [B]
struct TypeWork {
    size_t tn, B;
    TypeWork(int Nf, int nh, int B_) : tn((size_t)(Nf > 1 ? Nf : 1) * (size_t)nh), B((size_t)B_) {}
    size_t g0_h() const { return 0; }           size_t gs_h() const { return tn; }              size_t j_h() const { return 2 * tn; }
    size_t grad_h() const { return 3 * tn; }    size_t shift_h() const { return 4 * tn; }       size_t E_type() const { return 5 * tn; }
    size_t words() const { return 5 * tn + B; }
};

}  // namespace pfrestr
