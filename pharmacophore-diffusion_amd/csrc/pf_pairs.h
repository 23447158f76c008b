// Pair guidance of a guided run (pf_guide_pairs_next; semantics in include/pfdyn.h, "pair guidance", and DESIGN 4.25): distance
// restraints between two centers of one graph, a hinge below lo and above hi.
// This header is host only -- no HIP runtime call, no handle: the layout of the restraint block, every check of the caller's
// arrays against the bound batch, and the packing into the staging buffer (tests/pairs_check.cpp runs all three without a GPU).
// The block is not pf_restr.h's: it has no point and its hi column may be +inf, which validate_block refuses.  What the kernel
// reads is pf_device.h's PairParams.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#ifndef PF_PAIRS_MAX_PER_GRAPH
#define PF_PAIRS_MAX_PER_GRAPH 256      // pair restraints per graph (include/pfdyn.h states it too)
#endif
#define PF_PAIRS_MAX_CENTERS 64         // centers per graph k_guide_pairs stages (the bind's own limit)

namespace pfpairs {

// What the caller handed to pf_guide_pairs_next, as it came (host arrays; ptr may be NULL: no pair restraint in any graph)
struct PairsArgs {
    const int32_t* ptr; const int32_t* i; const int32_t* j;
    const float* lo; const float* hi; const float* w;
};

// The block (the device allocation and its staging buffer), in 32-bit words, n1 = max(n, 1), all of it uploaded:
//   ptr [B + 1]  i [n1]  j [n1]  lo [n1]  hi [n1]  w [n1]
struct PairsLayout {
    size_t B1, n1;
    PairsLayout(int B, int n) : B1((size_t)B + 1), n1((size_t)(n > 1 ? n : 1)) {}
    size_t ptr() const { return 0; }            size_t i() const { return B1; }                 size_t j() const { return B1 + n1; }
    size_t lo() const { return B1 + 2 * n1; }   size_t hi() const { return B1 + 3 * n1; }       size_t w() const { return B1 + 4 * n1; }
    size_t words() const { return B1 + 5 * n1; }
};

#define PF_PAIRS_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)

// Every check of pf_guide_pairs_next's arguments against the bound batch (B graphs, pharm_ptr [B + 1] its centers).  false: msg
// holds what was wrong; nothing else is written
inline bool validate(const PairsArgs& a, int B, const int32_t* pharm_ptr, char* msg, size_t msg_len) {
    const char* who = "pf_guide_pairs_next";
    if (B < 0 || !pharm_ptr) PF_PAIRS_BAD("%s: no batch to validate against", who);
    if (!a.ptr) return true;
    if (a.ptr[0] != 0) PF_PAIRS_BAD("%s: ptr[0] must be 0", who);
    for (int g = 0; g < B; ++g) {
        const int n = a.ptr[g + 1] - a.ptr[g];
        if (n < 0) PF_PAIRS_BAD("%s: ptr decreases at graph %d", who, g);
        if (n > PF_PAIRS_MAX_PER_GRAPH) PF_PAIRS_BAD("%s: graph %d has %d pair restraints (at most %d per graph)", who, g, n, PF_PAIRS_MAX_PER_GRAPH);
    }
    if (a.ptr[B] > 0 && (!a.i || !a.j || !a.lo || !a.hi || !a.w)) PF_PAIRS_BAD("%s: null pair restraint array", who);
    for (int g = 0; g < B; ++g) {
        const int nf_g = pharm_ptr[g + 1] - pharm_ptr[g];
        if (a.ptr[g + 1] > a.ptr[g] && nf_g > PF_PAIRS_MAX_CENTERS)
            PF_PAIRS_BAD("%s: graph %d has %d centers (pair restraints: at most %d per graph)", who, g, nf_g, PF_PAIRS_MAX_CENTERS);
        for (int k = a.ptr[g]; k < a.ptr[g + 1]; ++k) {
            for (const int32_t c : {a.i[k], a.j[k]})
                if (c < -1 || c >= nf_g)
                    PF_PAIRS_BAD("%s: pair restraint %d names center %d of graph %d, which has %d (-1: every center)", who, k, (int)c, g, nf_g);
            if (a.i[k] >= 0 && a.i[k] == a.j[k]) PF_PAIRS_BAD("%s: pair restraint %d names center %d twice", who, k, (int)a.i[k]);
            if (!(a.lo[k] >= 0.f) || !std::isfinite(a.lo[k])) PF_PAIRS_BAD("%s: pair restraint %d: lo must be finite and >= 0", who, k);
            if (!(a.hi[k] >= a.lo[k])) PF_PAIRS_BAD("%s: pair restraint %d: hi must be >= lo (+inf: no upper bound)", who, k);
            if (!(a.w[k] >= 0.f) || !std::isfinite(a.w[k])) PF_PAIRS_BAD("%s: pair restraint %d: the weight must be finite and >= 0", who, k);
        }
    }
    return true;
}
#undef PF_PAIRS_BAD

inline int n_restraints(const PairsArgs& a, int B) { return a.ptr ? a.ptr[B] : 0; }

// Validated arguments into the staging buffer, in the block's layout (words() words are written).  No ptr: no restraint in any
// graph
inline void pack(const PairsArgs& a, int B, uint32_t* st) {
    const int n = n_restraints(a, B);
    const PairsLayout pl(B, n);
    std::memset(st, 0, pl.words() * 4);
    if (!a.ptr) return;
    std::memcpy(st + pl.ptr(), a.ptr, pl.B1 * 4);
    if (n <= 0) return;
    const void* col[5] = {a.i, a.j, a.lo, a.hi, a.w};
    const size_t at[5] = {pl.i(), pl.j(), pl.lo(), pl.hi(), pl.w()};
    for (int k = 0; k < 5; ++k) std::memcpy(st + at[k], col[k], (size_t)n * 4);
}

// ---- what a step with pair restraints leaves, in 32-bit words (nf1 = max(Nf, 1)): next to pf_restr.h's GuideWork / TypeWork ----
// d_pguide:  g_pair [nf1][3]  E_pair [B]
struct PairWork {
    size_t nf1, B;
    PairWork(int Nf, int B_) : nf1((size_t)(Nf > 1 ? Nf : 1)), B((size_t)B_) {}
    size_t g_pair() const { return 0; }         size_t E_pair() const { return nf1 * 3; }       size_t words() const { return nf1 * 3 + B; }
};

}  // namespace pfpairs
