// The pocket field of a guided run (pf_guide_field_next; semantics in include/pfdyn.h, "pocket field", and DESIGN 4.22): the
// clash term over the graph's own atoms and the complementarity term over receptor features.  This header is host only -- no HIP
// runtime call, no handle: the layout of the field block, every check of the caller's arrays, and the packing into the staging
// buffer (tests/field_check.cpp runs all three without a GPU).  What the kernel of pf_field.hip reads is pf_device.h's FieldParams.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define PF_FIELD_MAX_FEATURES 4096      // receptor features per graph
#define PF_FIELD_MAX_TYPES 16           // pharm_nf (pf_create's own limit)

namespace pffield {

// What the caller handed to pf_guide_field_next, as it came (host arrays; atom_r / ph_ptr may be NULL: that term is absent)
struct FieldArgs {
    const float* atom_r; float w_clash;
    const int32_t* ph_ptr; const float* ph_x; const int32_t* ph_type;
    const int32_t* match; const float* dist;
    float w_comp, kappa, type_sharpness;
};

// The field block (the device allocation and its staging buffer), in 32-bit words:
//   ph_xt [n1][4]  atom_r [Np1]  ph_ptr [B + 1]  match [nt][nt]  dist [nt]  E3 [B][3]
// with Np1 = max(Np, 1), n1 = max(n, 1).  ph_xt: a receptor feature's position and, in the fourth word, its type (an integer's
// bits) -- one 16-byte load per feature, which is why it comes first.  E3 is device only (what the last step's launch left:
// restraints, clash, complementarity); the upload covers the words in front of it
struct FieldLayout {
    size_t Np1, B1, n1, nt;
    FieldLayout(int Np, int B, int n, int nt_) : Np1((size_t)(Np > 1 ? Np : 1)), B1((size_t)B + 1), n1((size_t)(n > 1 ? n : 1)), nt((size_t)nt_) {}
    size_t ph_xt() const { return 0; }
    size_t atom_r() const { return 4 * n1; }
    size_t ph_ptr() const { return 4 * n1 + Np1; }
    size_t match() const { return 4 * n1 + Np1 + B1; }
    size_t dist() const { return match() + nt * nt; }
    size_t upload_words() const { return dist() + nt; }
    size_t e3() const { return upload_words(); }
    size_t words() const { return e3() + (B1 - 1) * 3; }
};

#define PF_FIELD_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)

// Every check of pf_guide_field_next's arguments against the bound batch (B graphs, Np atoms, nt = pharm_nf feature types).
// false: msg holds what was wrong; nothing else is written
inline bool validate(const FieldArgs& a, int B, int Np, int nt, char* msg, size_t msg_len) {
    const char* who = "pf_guide_field_next";
    if (B < 0 || Np < 0 || nt < 1 || nt > PF_FIELD_MAX_TYPES) PF_FIELD_BAD("%s: no batch to validate against", who);
    if (!(a.w_clash >= 0.f) || !std::isfinite(a.w_clash)) PF_FIELD_BAD("%s: w_clash must be finite and >= 0", who);
    if (!(a.w_comp >= 0.f) || !std::isfinite(a.w_comp)) PF_FIELD_BAD("%s: w_comp must be finite and >= 0", who);
    if (!(a.kappa > 0.f) || !std::isfinite(a.kappa)) PF_FIELD_BAD("%s: kappa must be finite and > 0", who);
    if (!(a.type_sharpness >= 0.f) || !std::isfinite(a.type_sharpness)) PF_FIELD_BAD("%s: type_sharpness must be finite and >= 0", who);
    if (a.atom_r)
        for (int i = 0; i < Np; ++i)
            if (!(a.atom_r[i] >= 0.f) || !std::isfinite(a.atom_r[i])) PF_FIELD_BAD("%s: atom %d: the radius must be finite and >= 0", who, i);
    if (!a.ph_ptr) return true;
    if (!a.match || !a.dist) PF_FIELD_BAD("%s: receptor features need the match table and the distances", who);
    if (a.ph_ptr[0] != 0) PF_FIELD_BAD("%s: ph_ptr[0] must be 0", who);
    for (int g = 0; g < B; ++g) {
        const int n = a.ph_ptr[g + 1] - a.ph_ptr[g];
        if (n < 0) PF_FIELD_BAD("%s: ph_ptr decreases at graph %d", who, g);
        if (n > PF_FIELD_MAX_FEATURES) PF_FIELD_BAD("%s: graph %d has %d receptor features (at most %d per graph)", who, g, n, PF_FIELD_MAX_FEATURES);
    }
    const int n = a.ph_ptr[B];
    if (n > 0 && (!a.ph_x || !a.ph_type)) PF_FIELD_BAD("%s: null receptor feature array", who);
    for (int j = 0; j < n; ++j) {
        if (a.ph_type[j] < 0 || a.ph_type[j] >= nt) PF_FIELD_BAD("%s: receptor feature %d has type %d (0 .. %d)", who, j, (int)a.ph_type[j], nt - 1);
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(a.ph_x[(size_t)j * 3 + c])) PF_FIELD_BAD("%s: receptor feature %d has a non-finite position", who, j);
    }
    for (int t = 0; t < nt; ++t) {
        if (!(a.dist[t] >= 0.f) || !std::isfinite(a.dist[t])) PF_FIELD_BAD("%s: the distance of type %d must be finite and >= 0", who, t);
        for (int u = 0; u < nt; ++u)
            if (a.match[t * nt + u] != 0 && a.match[t * nt + u] != 1) PF_FIELD_BAD("%s: match[%d][%d] must be 0 or 1", who, t, u);
    }
    return true;
}
#undef PF_FIELD_BAD

inline int n_features(const FieldArgs& a, int B) { return a.ph_ptr ? a.ph_ptr[B] : 0; }

// Validated arguments into the staging buffer, in the block's layout (upload_words() words are written).  An absent clash term is
// radii of zero, an absent complementarity term is no feature in any graph: both contribute exact zeros
inline void pack(const FieldArgs& a, int B, int Np, int nt, uint32_t* st) {
    const int n = n_features(a, B);
    const FieldLayout fl(Np, B, n, nt);
    std::memset(st, 0, fl.upload_words() * 4);
    if (a.atom_r && Np > 0) std::memcpy(st + fl.atom_r(), a.atom_r, (size_t)Np * 4);
    if (!a.ph_ptr) return;
    std::memcpy(st + fl.ph_ptr(), a.ph_ptr, fl.B1 * 4);
    for (int j = 0; j < n; ++j) {
        std::memcpy(st + fl.ph_xt() + (size_t)j * 4, a.ph_x + (size_t)j * 3, 12);
        std::memcpy(st + fl.ph_xt() + (size_t)j * 4 + 3, a.ph_type + j, 4);
    }
    std::memcpy(st + fl.match(), a.match, (size_t)nt * nt * 4);
    std::memcpy(st + fl.dist(), a.dist, (size_t)nt * 4);
}

}  // namespace pffield
