// The guarded optimiser step on flat fp32 vectors of length n (pf_adam_step_guarded / pf_debug_optim_step): three launches on
// the caller's stream, no host synchronisation, no atomics, and no thread reads a word another thread of its launch writes.
//   k_optim_norm      one workgroup per chunk of PFO_CHUNK floats: sum of g[i]^2 in fp64 -- per thread its elements in ascending
//                     order, then the lanes of a wave (xor butterfly, widest stride first), then the four waves through LDS in
//                     ascending order -- one partial per chunk
//   k_optim_finalize  one workgroup: the partials summed in ascending order by one thread (staged through LDS 256 at a time),
//                     norm = (float)sqrt(sum); the finite flag, the clip coefficient, the two counters and the bias corrections
//                     of the APPLIED step count (1 - beta^t in double) go into the state block
//   k_adam_guarded    one workgroup per chunk: k_adam's arithmetic (pf_train.hip) on gi = g[i] * grad_scale * coef, clamped to
//                     [-clip, clip] under PF_CLIP_VALUE, plus the EMA stream and the mirror store; returns at once when the
//                     finite flag is off
// The finalising launch instead of a re-reduction of the partials inside every workgroup of k_adam_guarded: the counters need a
// launch of their own anyway (a workgroup that bumped them would write what the others read), and with it the Adam launch
// reads five words instead of n / PFO_CHUNK doubles per workgroup (DESIGN.md 4.21 has the timings).
// 16-byte loads and stores when every vector is 16-byte aligned, 4-byte ones otherwise; both forms give a thread the same
// elements, so the norm's bits do not depend on the alignment.
#include "pf_optim.h"

#include <cmath>

namespace {

// element e (0..15) of thread tid in a chunk: quad q = e / 4 of the thread sits at float (q * PFO_THREADS + tid) * 4 of the chunk
constexpr int kQuads = PFO_CHUNK / (4 * PFO_THREADS);
static_assert(kQuads * 4 * PFO_THREADS == PFO_CHUNK, "a chunk is a whole number of float4 rows of the workgroup");

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(PFO_THREADS) void k_optim_norm(const float* __restrict__ g, const size_t n, double* __restrict__ partials) {
    __shared__ double s_w[PFO_THREADS / 64];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * PFO_CHUNK;
    const bool vec = aligned16(g);
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < kQuads; ++q) {
        const size_t i = base + (size_t)(q * PFO_THREADS + tid) * 4;
        if (vec && i + 4 <= n) {
            const float4 x = *reinterpret_cast<const float4*>(g + i);
            acc = fma((double)x.x, (double)x.x, acc);
            acc = fma((double)x.y, (double)x.y, acc);
            acc = fma((double)x.z, (double)x.z, acc);
            acc = fma((double)x.w, (double)x.w, acc);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) { const double x = (double)g[i + k]; acc = fma(x, x, acc); }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = s_w[0];
#pragma unroll
        for (int w = 1; w < PFO_THREADS / 64; ++w) t += s_w[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(PFO_THREADS) void k_optim_finalize(const double* __restrict__ partials, const int n_part, OptimState* st,
                                                                const float grad_scale, const int clip_mode, const float clip,
                                                                const float b1, const float b2) {
    __shared__ double s_p[PFO_THREADS];
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int b = 0; b < n_part; b += PFO_THREADS) {
        s_p[tid] = b + tid < n_part ? partials[b + tid] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int m = min(PFO_THREADS, n_part - b);
#pragma unroll 8
            for (int k = 0; k < m; ++k) sum += s_p[k];      // (unrolled: the LDS reads of eight partials in flight, the adds in order)
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float norm = (float)sqrt(sum);
    const bool fin = isfinite(norm);
    const float ns = grad_scale * norm;                      // the norm of the gradient the step uses
    float coef = 1.0f;
    if (clip_mode == 1) coef = fminf(1.0f, clip / (ns + 1e-6f));          // torch.nn.utils.clip_grad_norm_
    long long applied = st->applied, skipped = st->skipped;
    if (fin) {
        ++applied;
        // beta^t by squaring, both chains interleaved (a few 2^-53 of relative error per squaring, far below the fp32 the
        // corrections are rounded to; two calls of the library pow are one thread's long dependent chain: 0.7 us of this launch)
        double pa = 1.0, pb = 1.0, qa = (double)b1, qb = (double)b2;
        for (long long t = applied; t; t >>= 1) {
            if (t & 1) { pa *= qa; pb *= qb; }
            qa *= qa; qb *= qb;
        }
        const double bc1 = 1.0 - pa, bc2 = 1.0 - pb;
        st->bc1 = (float)bc1;
        st->bc2_sqrt = (float)sqrt(bc2);
    } else {
        ++skipped;
        coef = 0.0f;
    }
    st->applied = applied;
    st->skipped = skipped;
    st->norm = ns;
    st->coef = coef;
    st->finite = fin ? 1 : 0;
}

struct AdamConst {
    float lr_bc1, b1, b2, eps, wd, scale, coef, bc2_sqrt, vclip, ema_w;
    bool clip_value;
};

// k_adam's arithmetic (pf_train.hip), line for line, behind the scaled / clipped gradient; returns the new parameter
__device__ __forceinline__ float adam_one(const AdamConst& c, const float g, const float pi, float& m, float& v) {
    float gi = __fmul_rn(__fmul_rn(g, c.scale), c.coef);
    if (c.clip_value) gi = fminf(fmaxf(gi, -c.vclip), c.vclip);
    if (c.wd != 0.f) gi = fmaf(c.wd, pi, gi);
    // k_adam's `m + (1 - b1) * (gi - m)` and `b2 * v + (1 - b2) * gi * gi` with the contractions the compiler makes there written
    // out, so that the moments keep k_adam's bits whatever surrounds these lines (tests/test_gpu_optim.py: exactness)
    const float mi = fmaf(1.0f - c.b1, gi - m, m);              // lerp, as torch
    const float vi = fmaf(c.b2, v, __fmul_rn(__fmul_rn(1.0f - c.b2, gi), gi));
    m = mi; v = vi;
    const float denom = sqrtf(vi) / c.bc2_sqrt + c.eps;
    return pi - c.lr_bc1 * (mi / denom);
}

__global__ __launch_bounds__(PFO_THREADS) void k_adam_guarded(const OptimParams P) {
    const OptimState* st = P.state;
    if (!st->finite) return;                                    // a skipped step writes nothing
    AdamConst c;
    c.lr_bc1 = P.lr / st->bc1; c.b1 = P.b1; c.b2 = P.b2; c.eps = P.eps; c.wd = P.wd; c.scale = P.grad_scale; c.coef = st->coef;
    c.bc2_sqrt = st->bc2_sqrt; c.vclip = P.clip; c.clip_value = P.clip_mode == 2; c.ema_w = 1.0f - P.ema_decay;
    const int tid = threadIdx.x;
    const size_t n = P.n, base = (size_t)blockIdx.x * PFO_CHUNK;
    const bool vec = aligned16(P.p) && aligned16(P.g) && aligned16(P.m) && aligned16(P.v) && aligned16(P.ema) && aligned16(P.mirror);
#pragma unroll
    for (int q = 0; q < kQuads; ++q) {
        const size_t i = base + (size_t)(q * PFO_THREADS + tid) * 4;
        if (vec && i + 4 <= n) {
            const float4 g4 = *reinterpret_cast<const float4*>(P.g + i);
            const float4 p4 = *reinterpret_cast<const float4*>(P.p + i);
            float4 m4 = *reinterpret_cast<const float4*>(P.m + i);
            float4 v4 = *reinterpret_cast<const float4*>(P.v + i);
            float4 o;
            o.x = adam_one(c, g4.x, p4.x, m4.x, v4.x);
            o.y = adam_one(c, g4.y, p4.y, m4.y, v4.y);
            o.z = adam_one(c, g4.z, p4.z, m4.z, v4.z);
            o.w = adam_one(c, g4.w, p4.w, m4.w, v4.w);
            *reinterpret_cast<float4*>(P.m + i) = m4;
            *reinterpret_cast<float4*>(P.v + i) = v4;
            *reinterpret_cast<float4*>(P.p + i) = o;
            if (P.mirror) *reinterpret_cast<float4*>(P.mirror + i) = o;
            if (P.ema) {
                float4 e = *reinterpret_cast<const float4*>(P.ema + i);
                e.x += c.ema_w * (o.x - e.x); e.y += c.ema_w * (o.y - e.y);
                e.z += c.ema_w * (o.z - e.z); e.w += c.ema_w * (o.w - e.w);
                *reinterpret_cast<float4*>(P.ema + i) = e;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t j = i + k;
                if (j >= n) break;
                float mj = P.m[j], vj = P.v[j];
                const float pn = adam_one(c, P.g[j], P.p[j], mj, vj);
                P.m[j] = mj; P.v[j] = vj; P.p[j] = pn;
                if (P.mirror) P.mirror[j] = pn;
                if (P.ema) { const float e = P.ema[j]; P.ema[j] = e + c.ema_w * (pn - e); }
            }
        }
    }
}

__global__ void k_optim_state_init(OptimState* st, const long long applied) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->applied = applied; st->skipped = 0;
    st->norm = 0.f; st->coef = 1.f; st->finite = 1;
    st->bc1 = 1.f; st->bc2_sqrt = 1.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) st->reserved[k] = 0;
}

}  // namespace

void pfk_optim_step(const OptimParams& p, hipStream_t s) {
    const unsigned nblk = (unsigned)((p.n + PFO_CHUNK - 1) / PFO_CHUNK);
    hipLaunchKernelGGL(k_optim_norm, dim3(nblk), dim3(PFO_THREADS), 0, s, p.g, p.n, p.partials);
    hipLaunchKernelGGL(k_optim_finalize, dim3(1), dim3(PFO_THREADS), 0, s, (const double*)p.partials, (int)nblk, p.state, p.grad_scale,
                       p.clip_mode, p.clip, p.b1, p.b2);
    hipLaunchKernelGGL(k_adam_guarded, dim3(nblk), dim3(PFO_THREADS), 0, s, p);
}

void pfk_optim_state_init(OptimState* state, long long applied, hipStream_t s) {
    hipLaunchKernelGGL(k_optim_state_init, dim3(1), dim3(64), 0, s, state, applied);
}
