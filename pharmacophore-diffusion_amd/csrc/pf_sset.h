// Analysis of a pocket's sample set (pf_sample_set_analyze; semantics in include/pfdyn.h, "sample sets", and DESIGN 4.26): typed
// Gaussian-overlap Tanimoto between the samples of a set, per-center support, Taylor-Butina clusters, consensus of each cluster.
// This header is host only -- no HIP runtime call, no handle: the layout of the packed block the kernels read, the plan of a
// call (where each set's matrix and work items start), every check of the caller's arrays and options, and the packing into the
// staging buffer (tests/sset_check.cpp runs all of it without a GPU).  What the kernels read is SsetParams below.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define PF_SSET_MAX_SAMPLES 1024                // samples per set (include/pfdyn.h states it too)
#define PF_SSET_MAX_CENTERS 64                  // centers per sample
#define PF_SSET_MAX_SIM ((int64_t)1 << 26)      // floats of all similarity matrices of one call: sum over the sets of S_p^2
#define PF_SSET_TILE 16                         // samples per LDS tile of k_sset_overlap: 16 x 16 sample pairs, one per thread

// the options of a call (include/pfdyn.h declares the same struct as pf_sset_opts)
struct pf_sset_opts_host { float sigma, tolerance, threshold; };

// What the three kernels read (passed by value).  ptr block (device, 32-bit words): SsetLayout below
struct SsetParams {
    int P, S, N, nf;                            // sets, samples, centers of the call; types are in [0, nf)
    const int32_t* set_ptr;                     // [P + 1] first sample of each set
    const int32_t* sim_ptr;                     // [P + 1] first float of each set's S_p x S_p matrix
    const int32_t* work_ptr;                    // [P + 1] first k_sset_overlap workgroup of each set (one per unordered tile pair)
    const int32_t* center_ptr;                  // [S + 1] first center of each sample
    const float* x;                             // [N, 3]
    const int32_t* type;                        // [N]
    float inv_2s2, tol2, threshold;             // 1 / (2 sigma^2), tolerance^2 (both rounded once from fp64), threshold
    float* sim;                                 // [sum S_p^2]
    int32_t* support;                           // [N]   zeroed before the launch
    int32_t* label;                             // [S]
    int32_t* centroid;                          // [S]   slot set_ptr[p] + c; -1 beyond n_clusters
    int32_t* size;                              // [S]
    int32_t* n_clusters;                        // [P]
    float* cons_x;                              // [N, 3] zeroed before the launch
    int32_t* cons_cnt;                          // [N]   zeroed before the launch
    int32_t* status;                            // [1]   number of centers whose type is outside [0, nf); zeroed before the launch
};

namespace pfsset {

// What the caller handed to pf_sample_set_analyze, as it came (host arrays)
struct SsetArgs {
    int P; const int32_t* set_ptr; const int32_t* center_ptr; const pf_sset_opts_host* opts;
};

// The packed block (the device allocation and its staging buffer), in 32-bit words, all of it uploaded:
//   set_ptr [P + 1]  sim_ptr [P + 1]  work_ptr [P + 1]  center_ptr [S + 1]
struct SsetLayout {
    size_t P1, S1;
    SsetLayout(int P, int S) : P1((size_t)P + 1), S1((size_t)S + 1) {}
    size_t set_ptr() const { return 0; }        size_t sim_ptr() const { return P1; }           size_t work_ptr() const { return 2 * P1; }
    size_t center_ptr() const { return 3 * P1; }
    size_t words() const { return 3 * P1 + S1; }
};

inline int tiles(int S) { return (S + PF_SSET_TILE - 1) / PF_SSET_TILE; }
inline int64_t tile_pairs(int S) { const int64_t t = tiles(S); return t * (t + 1) / 2; }

#define PF_SSET_BAD(...) do { std::snprintf(msg, msg_len, __VA_ARGS__); return false; } while (0)

// Every check of pf_sample_set_analyze's host arguments.  false: msg holds what was wrong; nothing else is written
inline bool validate(const SsetArgs& a, char* msg, size_t msg_len) {
    const char* who = "pf_sample_set_analyze";
    if (a.P < 1) PF_SSET_BAD("%s: %d sets (at least one)", who, a.P);
    if (!a.set_ptr || !a.center_ptr || !a.opts) PF_SSET_BAD("%s: null pointer array or options", who);
    const pf_sset_opts_host& o = *a.opts;
    if (!std::isfinite(o.sigma) || !(o.sigma > 0.f)) PF_SSET_BAD("%s: sigma must be finite and > 0", who);
    if (!std::isfinite(o.tolerance) || !(o.tolerance >= 0.f)) PF_SSET_BAD("%s: tolerance must be finite and >= 0", who);
    if (!(o.threshold >= 0.f && o.threshold <= 1.f)) PF_SSET_BAD("%s: threshold must be in [0, 1]", who);
    if (a.set_ptr[0] != 0) PF_SSET_BAD("%s: set_ptr[0] must be 0", who);
    int64_t sim = 0;
    for (int p = 0; p < a.P; ++p) {
        const int64_t S = (int64_t)a.set_ptr[p + 1] - a.set_ptr[p];
        if (S < 0) PF_SSET_BAD("%s: set_ptr decreases at set %d", who, p);
        if (S < 1 || S > PF_SSET_MAX_SAMPLES) PF_SSET_BAD("%s: set %d has %lld samples (1 to %d per set)", who, p, (long long)S, PF_SSET_MAX_SAMPLES);
        sim += S * S;
        if (sim > PF_SSET_MAX_SIM)
            PF_SSET_BAD("%s: the similarity matrices up to set %d hold %lld floats (at most %lld per call: split the call)", who, p, (long long)sim,
                        (long long)PF_SSET_MAX_SIM);
    }
    const int S = a.set_ptr[a.P];
    if (a.center_ptr[0] != 0) PF_SSET_BAD("%s: center_ptr[0] must be 0", who);
    for (int s = 0; s < S; ++s) {
        const int64_t n = (int64_t)a.center_ptr[s + 1] - a.center_ptr[s];
        if (n < 0) PF_SSET_BAD("%s: center_ptr decreases at sample %d", who, s);
        if (n < 1 || n > PF_SSET_MAX_CENTERS) PF_SSET_BAD("%s: sample %d has %lld centers (1 to %d per sample)", who, s, (long long)n, PF_SSET_MAX_CENTERS);
    }
    return true;
}
#undef PF_SSET_BAD

// The plan of a validated call: totals, and the scalars the kernels get
struct SsetPlan {
    int P, S, N;
    int64_t sim_floats, work_items;
    float inv_2s2, tol2, threshold;
};

inline SsetPlan plan(const SsetArgs& a) {
    SsetPlan pl{};
    pl.P = a.P; pl.S = a.set_ptr[a.P]; pl.N = a.center_ptr[pl.S];
    for (int p = 0; p < a.P; ++p) {
        const int64_t S = a.set_ptr[p + 1] - a.set_ptr[p];
        pl.sim_floats += S * S; pl.work_items += tile_pairs((int)S);
    }
    const double s = a.opts->sigma, t = a.opts->tolerance;
    pl.inv_2s2 = (float)(1.0 / (2.0 * s * s)); pl.tol2 = (float)(t * t); pl.threshold = a.opts->threshold;
    return pl;
}

// Validated arguments into the staging buffer, in the block's layout (words() words are written)
inline void pack(const SsetArgs& a, uint32_t* st) {
    const int S = a.set_ptr[a.P];
    const SsetLayout L(a.P, S);
    int32_t* w = reinterpret_cast<int32_t*>(st);
    std::memcpy(w + L.set_ptr(), a.set_ptr, L.P1 * 4);
    std::memcpy(w + L.center_ptr(), a.center_ptr, L.S1 * 4);
    int64_t sim = 0, work = 0;
    for (int p = 0; p <= a.P; ++p) {
        w[L.sim_ptr() + p] = (int32_t)sim; w[L.work_ptr() + p] = (int32_t)work;
        if (p == a.P) break;
        const int64_t Sp = a.set_ptr[p + 1] - a.set_ptr[p];
        sim += Sp * Sp; work += tile_pairs((int)Sp);
    }
}

}  // namespace pfsset
