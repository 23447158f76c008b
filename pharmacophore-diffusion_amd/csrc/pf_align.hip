// Rigid alignment of library entries onto queries (pf_pharm_align).  Two kernels on the caller's stream:
//   k_align_self    one thread per query / entry: its self overlap O_qq / O_ll, made once (every pair reads it), and the count of
//                   types outside [0, nf)
//   k_align_pairs   one wave (a workgroup of 64 threads) per (query, entry) pair
// A pair's seeds number from none to ~10^6 and each costs a 4 x 4 eigenproblem and up to 512 exponentials, while the filters that
// decide whether a candidate is a seed cost a few compares.  The wave therefore works in two alternating phases:
//   enumerate   the candidates of one query triplet i < j < k (wave-uniform) are spread as lane = (a, b), loop over c; the filter
//               votes are gathered with one ballot per c and the keys of the seeds that pass go into a ring of 128 in LDS, each at
//               its prefix count -- no atomics, and an (a, b) chunk without a type- and distance-compatible pair skips its c loop
//   solve       as soon as 64 keys wait (and once at the end for the rest) every lane takes one: transform (Horn's quaternion by
//               Jacobi sweeps in registers), overlap, and its own running best (O, key)
// so the solve phase runs with full lanes however few candidates pass.  A seed's overlap is made by one lane in one order and the
// best is reduced over (O, key) -- the larger O, on a tie the smaller key, which is the enumeration order -- so the winner does
// not depend on which lane or in which round a seed was solved.  The refinement (at most 16 short rounds) and the outputs are
// computed by every lane alike and written by the first lanes.  Query, entry, the entry's distance matrix and the type masks
// live in LDS (5.6 KiB); nothing is written to global memory but the pair's own outputs: plain vector stores, no floating-point
// atomics, one rounding per operation (FP contraction off) -- the same bits on every run, whatever else the call holds.
#include <hip/hip_runtime.h>
#include "pf_align.h"
#include "pf_align_core.h"

#define ALIGN_NQ PF_ALIGN_MAX_QUERY_CENTERS
#define ALIGN_NL PF_ALIGN_MAX_ENTRY_CENTERS
#define ALIGN_RING 128                          // at most 63 keys wait when up to 64 more are pushed

__global__ __launch_bounds__(256) void k_align_self(const AlignParams q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= q.Q + q.L) return;
    const bool is_q = e < q.Q;
    const int32_t* ptr = is_q ? q.q_ptr : q.l_ptr;
    const int s = is_q ? e : e - q.Q;
    const int f0 = ptr[s], n = min(ptr[s + 1] - f0, is_q ? ALIGN_NQ : ALIGN_NL);
    const float* x = (is_q ? q.qx : q.lx) + (size_t)f0 * 3;
    const int32_t* t = (is_q ? q.qt : q.lt) + f0;
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += (t[i] < 0 || t[i] >= q.nf) ? 1 : 0;
    if (bad) atomicAdd(q.status, bad);
    q.self[e] = align_self_overlap(n, x, t, q.inv_2s2);
}

__global__ __launch_bounds__(64) void k_align_pairs(const AlignParams q) {
    __shared__ float s_x[ALIGN_NQ * 3], s_y[ALIGN_NL * 3];
    __shared__ int s_t[ALIGN_NQ], s_u[ALIGN_NL];
    __shared__ unsigned s_mask[ALIGN_NL];
    __shared__ float s_dl[ALIGN_NL][ALIGN_NL + 1];
    __shared__ int s_ring[ALIGN_RING];
    const int lane = threadIdx.x;
    const int pair = blockIdx.x;
    const int qi = pair / q.L, li = pair - qi * q.L;
    const int q0 = q.q_ptr[qi], nq = min(max(q.q_ptr[qi + 1] - q0, 0), ALIGN_NQ);
    const int l0 = q.l_ptr[li], nl = min(max(q.l_ptr[li + 1] - l0, 0), ALIGN_NL);

    // ---- stage the pair ----
    if (lane < nq) {
        for (int e = 0; e < 3; ++e) s_x[lane * 3 + e] = q.qx[(size_t)(q0 + lane) * 3 + e];
        s_t[lane] = q.qt[q0 + lane];
    }
    if (lane < nl) {
        for (int e = 0; e < 3; ++e) s_y[lane * 3 + e] = q.lx[(size_t)(l0 + lane) * 3 + e];
        s_u[lane] = q.lt[l0 + lane];
    }
    __syncthreads();
    if (lane < nl) {
        unsigned m = 0u;
        for (int p = 0; p < nq; ++p) m |= (s_t[p] == s_u[lane]) ? (1u << p) : 0u;
        s_mask[lane] = m;
    }
    for (int e = lane; e < nl * nl; e += 64) {
        const int a = e / nl, b = e - a * nl;
        s_dl[a][b] = align_dist(s_y + a * 3, s_y + b * 3);
    }
    __syncthreads();
    const AlignPairView P{nq, nl, s_x, s_t, s_y, s_u, s_mask};

    float best_o = -1.f;
    int best_key = 0x7fffffff;
    int n_seeds = 0, head = 0, waiting = 0;             // wave-uniform
    // the solve phase: the first `cnt` waiting keys, one per lane
    auto solve = [&](int cnt) {
        if (lane < cnt) {
            const int key = s_ring[(head + lane) & (ALIGN_RING - 1)];
            AlignXf T;
            align_seed_xf(P, key, T);
            const float o = align_overlap(P, T, q.inv_2s2);
            if (o > best_o || (o == best_o && key < best_key)) { best_o = o; best_key = key; }
        }
        head = (head + cnt) & (ALIGN_RING - 1); waiting -= cnt;
    };

    // ---- enumerate ----
    for (int i = 0; i < nq; ++i) for (int j = i + 1; j < nq; ++j) for (int k = j + 1; k < nq; ++k) {
        const float* xi = s_x + i * 3; const float* xj = s_x + j * 3; const float* xk = s_x + k * 3;
        if (!(align_area(xi, xj, xk) >= q.min_area)) continue;
        const float d_ij = align_dist(xi, xj), d_ik = align_dist(xi, xk), d_jk = align_dist(xj, xk);
        const int ti = s_t[i], tj = s_t[j], tk = s_t[k];
        for (int ab0 = 0; ab0 < nl * nl; ab0 += 64) {
            const int ab = ab0 + lane;
            const int a = min(ab / nl, nl - 1), b = ab - (ab / nl) * nl;
            const bool ok_ab = ab < nl * nl && a != b && s_u[a] == ti && s_u[b] == tj && fabsf(d_ij - s_dl[a][b]) <= q.seed_tol;
            if (__ballot(ok_ab) == 0ull) continue;
            for (int c = 0; c < nl; ++c) {
                if (s_u[c] != tk) continue;
                bool ok = ok_ab && c != a && c != b && fabsf(d_ik - s_dl[a][c]) <= q.seed_tol && fabsf(d_jk - s_dl[b][c]) <= q.seed_tol;
                if (ok) ok = align_area(s_y + a * 3, s_y + b * 3, s_y + c * 3) >= q.min_area;
                const unsigned long long vote = __ballot(ok);
                if (vote == 0ull) continue;
                if (ok) {
                    const int at = waiting + __popcll(vote & ((1ull << lane) - 1ull));
                    s_ring[(head + at) & (ALIGN_RING - 1)] = align_key(i, j, k, a, b, c);
                }
                const int pushed = __popcll(vote);
                waiting += pushed; n_seeds += pushed;
                __syncthreads();
                if (waiting >= 64) { solve(64); __syncthreads(); }
            }
        }
    }
    if (waiting > 0) solve(waiting);

    // ---- the best seed of the wave: larger O, on a tie the earlier key ----
    for (int off = 32; off >= 1; off >>= 1) {
        const float o2 = __shfl_xor(best_o, off, 64);
        const int k2 = __shfl_xor(best_key, off, 64);
        if (o2 > best_o || (o2 == best_o && k2 < best_key)) { best_o = o2; best_key = k2; }
    }

    // ---- refinement and outputs: every lane alike ----
    AlignResult res;
    if (n_seeds > 0 && best_o >= 0.f) {
        AlignXf T;
        align_seed_xf(P, best_key, T);
        align_finish(P, T, best_o, q.refine, q.inv_2s2, q.tol2, q.self[qi], q.self[q.Q + li], res);
    } else {
        res.sim = 0.f; res.matched = 0;
        for (int e = 0; e < 12; ++e) res.xf[e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
    }
    if (lane == 0) { q.sim[pair] = res.sim; q.matched[pair] = res.matched; q.n_seeds[pair] = n_seeds; }
    if (q.transform && lane < 12) {
        float v = res.xf[0];
#pragma unroll
        for (int e = 1; e < 12; ++e) v = lane == e ? res.xf[e] : v;
        q.transform[(size_t)pair * 12 + lane] = v;
    }
}

extern "C" void pfk_pharm_align(const AlignParams* q, hipStream_t s) {
    if (q->Q <= 0 || q->L <= 0) return;
    hipLaunchKernelGGL(k_align_self, dim3((q->Q + q->L + 255) / 256), dim3(256), 0, s, *q);
    hipLaunchKernelGGL(k_align_pairs, dim3((unsigned)((int64_t)q->Q * q->L)), dim3(64), 0, s, *q);
}
