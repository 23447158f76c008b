// Rigid alignment of a pharmacophore library onto queries (pf_pharm_align; semantics in include/pfdyn.h, "pharmacophore alignment",
// and DESIGN 4.27): per (query, entry) pair the best of a discrete set of three-point superpositions by typed Gaussian overlap,
// refined by weighted least squares.  This header is host only -- no HIP runtime call, no handle: the layout of the packed block
// the kernels read, the plan of a call, every check of the caller's arrays and options, and the packing into the staging buffer
// (tests/align_check.cpp runs all of it without a GPU).  What the kernels read is AlignParams below; the arithmetic of a pair is
// pf_align_core.h.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define PF_ALIGN_MAX_QUERY_CENTERS 16           // centers per query (include/pfdyn.h states the three caps too)
#define PF_ALIGN_MAX_ENTRY_CENTERS 32           // centers per library entry
#define PF_ALIGN_MAX_PAIRS ((int64_t)1 << 24)   // Q * L of one call
#define PF_ALIGN_MAX_REFINE 16                  // refinement rounds

// the options of a call (include/pfdyn.h declares the same struct as pf_align_opts)
struct pf_align_opts_host { float sigma, tolerance; int32_t refine; float min_area; };

// What the two kernels read (passed by value).  ptr block (device, 32-bit words): AlignLayout below
struct AlignParams {
    int Q, L, nf, refine;                       // queries, entries; types are in [0, nf); refinement rounds
    const int32_t* q_ptr;                       // [Q + 1] first center of each query
    const int32_t* l_ptr;                       // [L + 1] first center of each entry
    const float* qx; const int32_t* qt;         // [Nq, 3], [Nq]
    const float* lx; const int32_t* lt;         // [Nl, 3], [Nl]
    float inv_2s2, tol2, seed_tol, min_area;    // 1 / (2 sigma^2), tolerance^2, 2 tolerance (each rounded once from fp64), min_area
    float* self;                                // [Q + L] self overlaps: the queries', then the entries' (workspace)
    float* sim;                                 // [Q, L]
    int32_t* matched;                           // [Q, L]
    int32_t* n_seeds;                           // [Q, L]
    float* transform;                           // [Q, L, 12] or null
    int32_t* status;                            // [1]   number of centers whose type is outside [0, nf); zeroed before the launch
};

namespace pfalign {

// What the caller handed to pf_pharm_align, as it came (host arrays)
struct AlignArgs {
    int Q; const int32_t* q_ptr; int L; const int32_t* l_ptr; const pf_align_opts_host* opts;
};

// The packed block (the device allocation and its staging buffer), in 32-bit words, all of it uploaded:
//   q_ptr [Q + 1]  l_ptr [L + 1]
struct AlignLayout {
    size_t Q1, L1;
    AlignLayout(int Q, int L) : Q1((size_t)Q + 1), L1((size_t)L + 1) {}
    size_t q_ptr() const { return 0; }          size_t l_ptr() const { return Q1; }
    size_t words() const { return Q1 + L1; }
};

#define PF_ALIGN_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)

inline bool validate_ptr(const char* who, const char* what, const char* one, int n, const int32_t* ptr, int cap, char* msg, size_t msg_len) {
    if (ptr[0] != 0) PF_ALIGN_BAD("%s: %s_ptr[0] must be 0", who, what);
    for (int s = 0; s < n; ++s) {
        const int64_t c = (int64_t)ptr[s + 1] - ptr[s];
        if (c < 0) PF_ALIGN_BAD("%s: %s_ptr decreases at %s %d", who, what, one, s);
        if (c < 1 || c > cap) PF_ALIGN_BAD("%s: %s %d has %lld centers (1 to %d per %s)", who, one, s, (long long)c, cap, one);
    }
    return true;
}

// Every check of pf_pharm_align's host arguments.  false: msg holds what was wrong; nothing else is written
inline bool validate(const AlignArgs& a, char* msg, size_t msg_len) {
    const char* who = "pf_pharm_align";
    if (a.Q < 1) PF_ALIGN_BAD("%s: %d queries (at least one)", who, a.Q);
    if (a.L < 1) PF_ALIGN_BAD("%s: %d library entries (at least one)", who, a.L);
    if (!a.q_ptr || !a.l_ptr || !a.opts) PF_ALIGN_BAD("%s: null pointer array or options", who);
    if ((int64_t)a.Q * a.L > PF_ALIGN_MAX_PAIRS)
        PF_ALIGN_BAD("%s: %d queries x %d entries are %lld pairs (at most %lld per call: split the call)", who, a.Q, a.L,
                     (long long)((int64_t)a.Q * a.L), (long long)PF_ALIGN_MAX_PAIRS);
    const pf_align_opts_host& o = *a.opts;
    if (!std::isfinite(o.sigma) || !(o.sigma > 0.f)) PF_ALIGN_BAD("%s: sigma must be finite and > 0", who);
    if (!std::isfinite(o.tolerance) || !(o.tolerance >= 0.f)) PF_ALIGN_BAD("%s: tolerance must be finite and >= 0", who);
    if (o.refine < 0 || o.refine > PF_ALIGN_MAX_REFINE) PF_ALIGN_BAD("%s: refine must be in [0, %d], got %d", who, PF_ALIGN_MAX_REFINE, (int)o.refine);
    if (!std::isfinite(o.min_area) || !(o.min_area > 0.f)) PF_ALIGN_BAD("%s: min_area must be finite and > 0", who);
    if (!validate_ptr(who, "q", "query", a.Q, a.q_ptr, PF_ALIGN_MAX_QUERY_CENTERS, msg, msg_len)) return false;
    if (!validate_ptr(who, "l", "entry", a.L, a.l_ptr, PF_ALIGN_MAX_ENTRY_CENTERS, msg, msg_len)) return false;
    return true;
}
#undef PF_ALIGN_BAD

// The plan of a validated call: totals, and the scalars the kernels get
struct AlignPlan {
    int Q, L, Nq, Nl;
    int64_t pairs;                              // work items of k_align_pairs: one wave each
    int refine;
    float inv_2s2, tol2, seed_tol, min_area;
};

inline AlignPlan plan(const AlignArgs& a) {
    AlignPlan pl{};
    pl.Q = a.Q; pl.L = a.L; pl.Nq = a.q_ptr[a.Q]; pl.Nl = a.l_ptr[a.L];
    pl.pairs = (int64_t)a.Q * a.L;
    const double s = a.opts->sigma, t = a.opts->tolerance;
    pl.inv_2s2 = (float)(1.0 / (2.0 * s * s)); pl.tol2 = (float)(t * t); pl.seed_tol = (float)(2.0 * t);
    pl.min_area = a.opts->min_area; pl.refine = a.opts->refine;
    return pl;
}

// Validated arguments into the staging buffer, in the block's layout (words() words are written)
inline void pack(const AlignArgs& a, uint32_t* st) {
    const AlignLayout lay(a.Q, a.L);
    int32_t* w = reinterpret_cast<int32_t*>(st);
    std::memcpy(w + lay.q_ptr(), a.q_ptr, lay.Q1 * 4);
    std::memcpy(w + lay.l_ptr(), a.l_ptr, lay.L1 * 4);
}

}  // namespace pfalign
