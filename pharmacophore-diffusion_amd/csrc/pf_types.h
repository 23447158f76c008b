// Type guidance of a guided run (pf_guide_types_next; semantics in include/pfdyn.h, "type guidance", and DESIGN 4.24): typed
// restraints on the predicted clean feature rows and the switch that gives the complementarity energy its feature gradient.
// This header is host only -- no HIP runtime call, no handle: the layout of the restraint block, every check of the caller's
// arrays, and the packing into the staging buffer (tests/types_check.cpp runs all three without a GPU).  The block is the one the
// spatial restraints use (pf_restr.h); here are the names of its columns, the scalars' checks and the type column's.  What the
// kernels read is pf_device.h's TypeParams.
#pragma once
#include "pf_restr.h"

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

// The restraint block (the device allocation and its staging buffer) is pf_restr.h's, its integer columns named center, type:
//   ptr [B + 1]  center [n1]  type [n1]  p [n1][3]  r [n1]  w [n1]
struct TypesLayout : pfrestr::BlockLayout { using BlockLayout::BlockLayout; size_t center() const { return col_a(); } size_t type() const { return col_b(); } };
inline pfrestr::Block block(const TypesArgs& a) { return pfrestr::Block{a.ptr, a.center, a.type, a.p, a.r, a.w}; }

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
    const pfrestr::Words t{who, "type restraint", "ptr"};
    return pfrestr::validate_block(block(a), a.center, B, pharm_ptr, t, [&](int j, char* msg, size_t msg_len) {
        if (a.type[j] < 0 || a.type[j] >= nt) PF_TYPES_BAD("%s: type restraint %d has type %d (0 .. %d)", who, j, (int)a.type[j], nt - 1);
        return true;
    }, msg, msg_len);
}
#undef PF_TYPES_BAD

inline int n_restraints(const TypesArgs& a, int B) { return a.ptr ? a.ptr[B] : 0; }

// Validated arguments into the staging buffer, in the block's layout (words() words are written).  No restraint array: no
// restraint in any graph
inline void pack(const TypesArgs& a, int B, uint32_t* st) { pfrestr::pack_block(block(a), B, st); }

}  // namespace pftypes
