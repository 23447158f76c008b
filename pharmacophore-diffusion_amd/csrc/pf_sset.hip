// Analysis of sample sets (pf_sample_set_analyze): all samples of a pocket live in the pocket's frame, so two samples
// compare without alignment.  Three kernels on the caller's stream, many sets per launch:
//   k_sset_overlap    O(a,b) = sum_i sum_j [t_ai == t_bj] exp(-|x_ai - x_bj|^2 / (2 sigma^2)), sim = O(a,b) / (O(a,a) + O(b,b) - O(a,b)),
//                     support(a,i) = number of samples b != a with a center of type t_ai within the tolerance of x_ai
//   k_sset_cluster    Taylor-Butina on the matrix as written: neighbour counts, visit order (-count, index), two barriers per centroid
//   k_sset_consensus  per cluster and center of its centroid: the nearest same-type center within the tolerance in every member
// k_sset_overlap's work item is an unordered pair of 16-sample tiles of one set: both tiles are staged in LDS (x, y, z, type per
// center, rows of 65 words: the 16 rows a wave reads side by side fall into 16 different banks) and thread (ia, ib) is the sample
// pair -- every lane works whether a sample has 1 center or 64, where a wave per sample pair would idle 58 lanes at 6 centers.
// The self overlaps of the 32 staged samples are made first, 8 threads per sample (rows i = k mod 8, the partials summed k
// ascending), by every work item with the same operations: a sample's O(a,a) has the same bits wherever it is made.  Each
// unordered pair is computed once, in the self overlap's order (eight partials by row i mod 8 of a, j over b's centers inside),
// clamped to 1 and stored to both places; the diagonal is written as 1.0f.  Support counts are integers: LDS atomics per tile,
// one global atomic per staged center, any order.
// One rounding per operation (FP contraction off), plain vector stores: every output has the same bits on every run.
#include <hip/hip_runtime.h>
#include "pf_sset.h"

#define SSET_T PF_SSET_TILE
#define SSET_ROW (PF_SSET_MAX_CENTERS + 1)

// the set a work item / slot belongs to: the last p with ptr[p] <= k (ptr ascending, ptr[0] = 0, k < ptr[P])
__device__ __forceinline__ int sset_find(const int32_t* ptr, int P, int k) {
    int lo = 0, hi = P;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ptr[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void k_sset_overlap(const SsetParams q) {
    __shared__ float s_x[2][SSET_T][SSET_ROW], s_y[2][SSET_T][SSET_ROW], s_z[2][SSET_T][SSET_ROW];
    __shared__ int s_t[2][SSET_T][SSET_ROW];
    __shared__ int s_n[2][SSET_T];
    __shared__ int s_sup[2][SSET_T][PF_SSET_MAX_CENTERS];
    __shared__ float s_part[2 * SSET_T][8];
    __shared__ float s_self[2 * SSET_T];
    const int tid = threadIdx.x;
    const int p = sset_find(q.work_ptr, q.P, (int)blockIdx.x);
    const int s0 = q.set_ptr[p], S = q.set_ptr[p + 1] - s0;
    const int nt = (S + SSET_T - 1) / SSET_T;
    int k = (int)blockIdx.x - q.work_ptr[p], ta = 0;
    while (k >= nt - ta) { k -= nt - ta; ++ta; }
    const int tb = ta + k;
    const bool diag = ta == tb;
    float* sim = q.sim + q.sim_ptr[p];

    // ---- stage both tiles (a diagonal item stages its tile twice: one code path) ----
    if (tid < 2 * SSET_T) {
        const int side = tid / SSET_T, r = tid % SSET_T, a = (side ? tb : ta) * SSET_T + r;
        s_n[side][r] = a < S ? min(q.center_ptr[s0 + a + 1] - q.center_ptr[s0 + a], PF_SSET_MAX_CENTERS) : 0;
    }
    for (int e = tid; e < 2 * SSET_T * PF_SSET_MAX_CENTERS; e += 256)
        s_sup[e / (SSET_T * PF_SSET_MAX_CENTERS)][(e / PF_SSET_MAX_CENTERS) % SSET_T][e % PF_SSET_MAX_CENTERS] = 0;
    __syncthreads();
    int bad = 0;
    for (int e = tid; e < 2 * SSET_T * PF_SSET_MAX_CENTERS; e += 256) {
        const int side = e / (SSET_T * PF_SSET_MAX_CENTERS), r = (e / PF_SSET_MAX_CENTERS) % SSET_T, c = e % PF_SSET_MAX_CENTERS;
        if (c < s_n[side][r]) {
            const int a = (side ? tb : ta) * SSET_T + r;
            const size_t f = (size_t)q.center_ptr[s0 + a] + c;
            const int t = q.type[f];
            s_x[side][r][c] = q.x[f * 3]; s_y[side][r][c] = q.x[f * 3 + 1]; s_z[side][r][c] = q.x[f * 3 + 2];
            s_t[side][r][c] = t;
            if (diag && side == 0 && (t < 0 || t >= q.nf)) ++bad;        // each sample is side 0 of exactly one diagonal item
        }
    }
    if (bad) atomicAdd(q.status, bad);
    __syncthreads();

    // ---- self overlaps: sample w = tid / 8 of the 32 staged, rows i = k8 mod 8 ----
    {
#pragma clang fp contract(off)
        const int w = tid >> 3, k8 = tid & 7, side = w / SSET_T, r = w % SSET_T, n = s_n[side][r];
        float o = 0.f;
        for (int i = k8; i < n; i += 8) {
            const float xi = s_x[side][r][i], yi = s_y[side][r][i], zi = s_z[side][r][i];
            const int ti = s_t[side][r][i];
            for (int j = 0; j < n; ++j) {
                if (s_t[side][r][j] != ti) continue;
                const float dx = xi - s_x[side][r][j], dy = yi - s_y[side][r][j], dz = zi - s_z[side][r][j];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                o += expf(-(d2 * q.inv_2s2));
            }
        }
        s_part[w][k8] = o;
    }
    __syncthreads();
    if (tid < 2 * SSET_T) {
#pragma clang fp contract(off)
        float o = 0.f;
        for (int k8 = 0; k8 < 8; ++k8) o += s_part[tid][k8];
        s_self[tid] = o;
    }
    __syncthreads();

    // ---- thread (ia, ib): the pair of sample a = ta * 16 + ia and b = tb * 16 + ib ----
    {
#pragma clang fp contract(off)
        const int ia = tid / SSET_T, ib = tid % SSET_T;
        const int a = ta * SSET_T + ia, b = tb * SSET_T + ib;
        const int na = s_n[0][ia], nb = s_n[1][ib];
        if (a < S && b < S && (!diag || ia < ib)) {
            // eight partial sums by row i mod 8, met k ascending: the self overlap's order, so that O(a,b) of two identical
            // samples has O(a,a)'s bits and their similarity is exactly 1
            float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            unsigned long long hit_b = 0ull;                    // bit j: b's center j has a partner in a
            for (int i0 = 0; i0 < na; i0 += 8) {
#pragma unroll
                for (int k8 = 0; k8 < 8; ++k8) {
                    const int i = i0 + k8;
                    if (i >= na) break;
                    const float xi = s_x[0][ia][i], yi = s_y[0][ia][i], zi = s_z[0][ia][i];
                    const int ti = s_t[0][ia][i];
                    bool hit_a = false;
                    for (int j = 0; j < nb; ++j) {
                        if (s_t[1][ib][j] != ti) continue;
                        const float dx = xi - s_x[1][ib][j], dy = yi - s_y[1][ib][j], dz = zi - s_z[1][ib][j];
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        part[k8] += expf(-(d2 * q.inv_2s2));
                        if (d2 <= q.tol2) { hit_a = true; hit_b |= 1ull << j; }
                    }
                    if (hit_a) atomicAdd(&s_sup[0][ia][i], 1);
                }
            }
            float o = 0.f;
#pragma unroll
            for (int k8 = 0; k8 < 8; ++k8) o += part[k8];
            for (int j = 0; j < nb; ++j)
                if ((hit_b >> j) & 1ull) atomicAdd(&s_sup[1][ib][j], 1);
            const float den = (s_self[ia] + s_self[SSET_T + ib]) - o;
            const float v = fminf(o / den, 1.0f);               // (rounding may carry two near-identical samples an ulp past 1)
            sim[(size_t)a * S + b] = v;
            sim[(size_t)b * S + a] = v;
        } else if (diag && ia == ib && a < S) {
            sim[(size_t)a * S + a] = 1.0f;
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * SSET_T * PF_SSET_MAX_CENTERS; e += 256) {
        const int side = e / (SSET_T * PF_SSET_MAX_CENTERS), r = (e / PF_SSET_MAX_CENTERS) % SSET_T, c = e % PF_SSET_MAX_CENTERS;
        const int v = s_sup[side][r][c];
        if (v != 0 && c < s_n[side][r]) {
            const int a = (side ? tb : ta) * SSET_T + r;
            atomicAdd(&q.support[(size_t)q.center_ptr[s0 + a] + c], v);
        }
    }
}

// One workgroup per set.  Thread t owns the samples a = t, t + 256, ...  count(a) reads column a of the (bitwise symmetric)
// matrix, so the threads of a wave read side by side.  rank(a) = number of samples in front of a in the order (-count, index);
// the walk then visits order[0], order[1], ...: labelled samples are passed without a barrier, an unlabelled one becomes a
// centroid and takes its unlabelled neighbours between two barriers -- one behind every thread's decision (the labels it read
// were written in front of the previous centroid's closing barrier), one behind the cluster's label writes.
__global__ __launch_bounds__(256) void k_sset_cluster(const SsetParams q) {
    __shared__ int s_cnt[PF_SSET_MAX_SAMPLES], s_order[PF_SSET_MAX_SAMPLES], s_label[PF_SSET_MAX_SAMPLES], s_size[PF_SSET_MAX_SAMPLES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int s0 = q.set_ptr[p], S = min(q.set_ptr[p + 1] - s0, PF_SSET_MAX_SAMPLES);
    const float* sim = q.sim + q.sim_ptr[p];
    const float thr = q.threshold;
    for (int a = tid; a < S; a += 256) {
        int c = 0;
        for (int b = 0; b < S; ++b) c += (b != a && sim[(size_t)b * S + a] >= thr) ? 1 : 0;
        s_cnt[a] = c; s_label[a] = -1; s_size[a] = 0;
    }
    __syncthreads();
    for (int a = tid; a < S; a += 256) {
        const int ca = s_cnt[a];
        int r = 0;
        for (int b = 0; b < S; ++b) { const int cb = s_cnt[b]; r += (cb > ca || (cb == ca && b < a)) ? 1 : 0; }
        s_order[r] = a;
    }
    __syncthreads();
    int ncl = 0;
    for (int v = 0;; ++v) {
        // every thread finds the next unlabelled sample of the order for itself: no label changes between the barrier behind the
        // last centroid's writes and the barrier below, so all threads read the same words and agree on v
        while (v < S && s_label[s_order[v]] >= 0) ++v;
        if (v >= S) break;
        const int a = s_order[v];
        __syncthreads();                        // every thread has made its decision before the first label of this cluster is written
        int took = 0;
        for (int b = tid; b < S; b += 256)
            if (s_label[b] < 0 && (b == a || sim[(size_t)a * S + b] >= thr)) { s_label[b] = ncl; ++took; }
        if (took) atomicAdd(&s_size[ncl], took);
        if (tid == 0) q.centroid[s0 + ncl] = a;
        ++ncl;
        __syncthreads();                        // the cluster's labels are written before the next decision reads them
    }
    for (int a = tid; a < S; a += 256) {
        q.label[s0 + a] = s_label[a];
        q.size[s0 + a] = a < ncl ? s_size[a] : -1;
        if (a >= ncl) q.centroid[s0 + a] = -1;
    }
    if (tid == 0) q.n_clusters[p] = ncl;
}

// One workgroup per cluster slot (a sample index of the call), one thread per center of the slot's centroid sample.  The
// members are walked in ascending index, each staged in LDS once; thread i keeps the nearest same-type center within the
// tolerance (the lowest j of equals) and adds it to its own fp32 sum: one thread, one order.
__global__ __launch_bounds__(PF_SSET_MAX_CENTERS) void k_sset_consensus(const SsetParams q) {
    __shared__ float s_c[PF_SSET_MAX_CENTERS][3];
    __shared__ int s_t[PF_SSET_MAX_CENTERS];
    const int slot = blockIdx.x, i = threadIdx.x;
    const int p = sset_find(q.set_ptr, q.P, slot);
    const int s0 = q.set_ptr[p], S = q.set_ptr[p + 1] - s0, c = slot - s0;
    if (c >= q.n_clusters[p]) return;
    const int m = q.centroid[slot];
    const int f0 = q.center_ptr[s0 + m], n = min(q.center_ptr[s0 + m + 1] - f0, PF_SSET_MAX_CENTERS);
    const bool own = i < n;
    float x[3] = {0.f, 0.f, 0.f};
    int t = -1;
    if (own) { for (int k = 0; k < 3; ++k) x[k] = q.x[(size_t)(f0 + i) * 3 + k]; t = q.type[f0 + i]; }
    float pos[3] = {0.f, 0.f, 0.f};
    int cnt = 0;
    for (int b = 0; b < S; ++b) {
        if (q.label[s0 + b] != c) continue;
        const int g0 = q.center_ptr[s0 + b], nb = min(q.center_ptr[s0 + b + 1] - g0, PF_SSET_MAX_CENTERS);
        __syncthreads();
        if (i < nb) { for (int k = 0; k < 3; ++k) s_c[i][k] = q.x[(size_t)(g0 + i) * 3 + k]; s_t[i] = q.type[g0 + i]; }
        __syncthreads();
        if (own) {
#pragma clang fp contract(off)
            int best = -1;
            float best_d2 = 0.f;
            for (int j = 0; j < nb; ++j) {
                if (s_t[j] != t) continue;
                const float dx = x[0] - s_c[j][0], dy = x[1] - s_c[j][1], dz = x[2] - s_c[j][2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= q.tol2 && (best < 0 || d2 < best_d2)) { best = j; best_d2 = d2; }
            }
            if (best >= 0) { ++cnt; for (int k = 0; k < 3; ++k) pos[k] += s_c[best][k]; }
        }
    }
    if (own && cnt > 0) {
#pragma clang fp contract(off)
        const float fc = (float)cnt;
        for (int k = 0; k < 3; ++k) q.cons_x[(size_t)(f0 + i) * 3 + k] = pos[k] / fc;
        q.cons_cnt[f0 + i] = cnt;
    }
}

extern "C" void pfk_sset_analyze(const SsetParams* q, int work_items, hipStream_t s) {
    if (q->P <= 0 || q->S <= 0) return;
    hipLaunchKernelGGL(k_sset_overlap, dim3(work_items), dim3(256), 0, s, *q);
    hipLaunchKernelGGL(k_sset_cluster, dim3(q->P), dim3(256), 0, s, *q);
    hipLaunchKernelGGL(k_sset_consensus, dim3(q->S), dim3(PF_SSET_MAX_CENTERS), 0, s, *q);
}
