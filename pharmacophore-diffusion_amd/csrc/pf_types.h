// Type guidance of a guided run (pf_guide_types_next; semantics in include/pfdyn.h, "type guidance", and DESIGN 4.24): typed
// restraints on the predicted clean feature rows and the switch that gives the complementarity energy its feature gradient.
// This header is host only -- no HIP runtime call, no handle: the layout of the restraint block, every check of the caller's
// arrays, and the packing into the staging buffer (tests/types_check.cpp runs all three without a GPU).  What the kernels read is
// pf_device.h's TypeParams.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define PF_TYPES_MAX_PER_GRAPH 256      // type restraints per graph
#define PF_TYPES_MAX_TYPES 16           // pharm_nf (pf_create's own limit)

namespace pftypes {

// What the caller handed to pf_guide_types_next, as it came (host arrays; ptr may be NULL: no type restraint in any graph)
struct TypesArgs {
    const int32_t* ptr; const int32_t* center; const int32_t* type;
    const float* p; const float* r; const float* w;
    float feat_scale, feat_clip, type_sharpness;
    int32_t comp_types;
    float unmatched;
};

// The restraint block (the device allocation and its staging buffer), in 32-bit words:
//   ptr [B + 1]  center [n1]  type [n1]  p [n1][3]  r [n1]  w [n1]
// with n1 = max(n, 1).  All of it is uploaded
struct TypesLayout {
    size_t B1, n1;
    TypesLayout(int B, int n) : B1((size_t)B + 1), n1((size_t)(n > 1 ? n : 1)) {}
    size_t ptr() const { return 0; }
    size_t center() const { return B1; }
    size_t type() const { return B1 + n1; }
    size_t p() const { return B1 + 2 * n1; }
    size_t r() const { return B1 + 5 * n1; }
    size_t w() const { return B1 + 6 * n1; }
    size_t words() const { return B1 + 7 * n1; }
};

#define PF_TYPES_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)

// Every check of pf_guide_types_next's arguments against the bound batch (B graphs, pharm_ptr [B + 1] its centers, nt = pharm_nf
// feature types).  false: msg holds what was wrong; nothing else is written
inline bool validate(const TypesArgs& a, int B, const int32_t* pharm_ptr, int nt, char* msg, size_t msg_len) {
    const char* who = "pf_guide_types_next";
    if (B < 0 || !pharm_ptr || nt < 1 || nt > PF_TYPES_MAX_TYPES) PF_TYPES_BAD("%s: no batch to validate against", who);
    if (!(a.feat_scale >= 0.f) || !std::isfinite(a.feat_scale)) PF_TYPES_BAD("%s: feat_scale must be finite and >= 0", who);
    if (!(a.feat_clip >= 0.f) || !std::isfinite(a.feat_clip)) PF_TYPES_BAD("%s: feat_clip must be finite and >= 0 (0: no clip)", who);
    if (!(a.type_sharpness >= 0.f) || !std::isfinite(a.type_sharpness)) PF_TYPES_BAD("%s: type_sharpness must be finite and >= 0", who);
    if (!(a.unmatched >= 0.f) || !std::isfinite(a.unmatched)) PF_TYPES_BAD("%s: unmatched must be finite and >= 0", who);
    if (a.comp_types != 0 && a.comp_types != 1) PF_TYPES_BAD("%s: comp_types must be 0 or 1", who);
    if (!a.ptr) return true;
    if (a.ptr[0] != 0) PF_TYPES_BAD("%s: ptr[0] must be 0", who);
    for (int g = 0; g < B; ++g) {
        const int n = a.ptr[g + 1] - a.ptr[g];
        if (n < 0) PF_TYPES_BAD("%s: ptr decreases at graph %d", who, g);
        if (n > PF_TYPES_MAX_PER_GRAPH) PF_TYPES_BAD("%s: graph %d has %d type restraints (at most %d per graph)", who, g, n, PF_TYPES_MAX_PER_GRAPH);
    }
    const int n = a.ptr[B];
    if (n > 0 && (!a.center || !a.type || !a.p || !a.r || !a.w)) PF_TYPES_BAD("%s: null type restraint array", who);
    for (int g = 0; g < B; ++g) {
        const int nf_g = pharm_ptr[g + 1] - pharm_ptr[g];
        for (int j = a.ptr[g]; j < a.ptr[g + 1]; ++j) {
            if (a.center[j] < -1 || a.center[j] >= nf_g)
                PF_TYPES_BAD("%s: type restraint %d names center %d of graph %d, which has %d (-1: every center)", who, j, (int)a.center[j], g, nf_g);
            if (a.type[j] < 0 || a.type[j] >= nt) PF_TYPES_BAD("%s: type restraint %d has type %d (0 .. %d)", who, j, (int)a.type[j], nt - 1);
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(a.p[(size_t)j * 3 + c])) PF_TYPES_BAD("%s: type restraint %d has a non-finite point", who, j);
            if (!(a.r[j] >= 0.f) || !std::isfinite(a.r[j])) PF_TYPES_BAD("%s: type restraint %d: the radius must be finite and >= 0", who, j);
            if (!(a.w[j] >= 0.f) || !std::isfinite(a.w[j])) PF_TYPES_BAD("%s: type restraint %d: the weight must be finite and >= 0", who, j);
        }
    }
    return true;
}
#undef PF_TYPES_BAD

inline int n_restraints(const TypesArgs& a, int B) { return a.ptr ? a.ptr[B] : 0; }

// Validated arguments into the staging buffer, in the block's layout (words() words are written).  No restraint array: no
// restraint in any graph
inline void pack(const TypesArgs& a, int B, uint32_t* st) {
    const int n = n_restraints(a, B);
    const TypesLayout tl(B, n);
    std::memset(st, 0, tl.words() * 4);
    if (!a.ptr || n == 0) return;
    std::memcpy(st + tl.ptr(), a.ptr, tl.B1 * 4);
    std::memcpy(st + tl.center(), a.center, (size_t)n * 4);
    std::memcpy(st + tl.type(), a.type, (size_t)n * 4);
    std::memcpy(st + tl.p(), a.p, (size_t)n * 12);
    std::memcpy(st + tl.r(), a.r, (size_t)n * 4);
    std::memcpy(st + tl.w(), a.w, (size_t)n * 4);
}

}  // namespace pftypes
