// Scoring given pharmacophores against a pocket (pf_score): the two small kernels around the inference forward of one noise level.
//   k_score_prepare (one block per graph): the arithmetic of k_loss_prepare (pf_train.hip; pharmacodiff.py:176-205) with ONE level
//     for the whole batch and the level's noise in the sampler's layout -- the COM of the clean centers is taken off the centers
//     and off the graph's pocket, z_t = alpha_t x0 + sigma_t eps (the features: h0 / feat_norm), the COM of the noised centers is
//     removed when remove_com; writes the dynamics' input state (xn, pharm_h) in place.  The pocket always starts from the bound
//     coordinates, whatever the level before left in xn
//   k_score_eval<EPC, EPF> (one wave per graph, fixed reduction order): the four forms of k_loss_eval<EPC, EPF> (:208-241) summed
//     over the centers of the graph instead of over the batch -- terms[g] = {pos, feat, err, hits} -- and
//     score[g] (+)= {w_pos * pos, w_feat * feat}.  It needs no scratch of the prepare kernel: the COM-removed clean center and the
//     second COM are recomputed by the same function (score_center: no contraction, one rounding per operation, so both kernels
//     get the same bits)
// A graph has at most 64 centers (the bind's limit) and pharm_nf <= 8 (the host entry refuses more): one lane per center.
#include "pf_score.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Lane `lane` of a full wave holds center f0 + lane of a graph with nfg centers (idle lanes carry zeros).  xc: the clean center
// minus the COM of the graph's clean centers (c1); xt: alpha xc + sigma eps_x minus the COM of those values (c2; zero without
// remove_com).  Every lane of the wave must call it.
__device__ __forceinline__ void score_center(const ScoreParams& p, const int f0, const int nfg, const int lane, const float a,
                                             const float sg, float (&xc)[3], float (&xt)[3], float (&c1)[3], float (&c2)[3]) {
    const bool on = lane < nfg;
    const size_t f = (size_t)f0 + (on ? lane : 0);
    const int row = 3 + p.nf;
    const float cnt = (float)max(nfg, 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = on ? p.x0[3 * f + c] : 0.f;
        const float e = on ? p.noise[f * row + c] : 0.f;
        c1[c] = wave_sum(x) / cnt;
        xc[c] = on ? __fsub_rn(x, c1[c]) : 0.f;
        const float z = on ? __fadd_rn(__fmul_rn(a, xc[c]), __fmul_rn(sg, e)) : 0.f;
        c2[c] = p.remove_com ? wave_sum(z) / cnt : 0.f;
        xt[c] = __fsub_rn(z, c2[c]);
    }
}

__global__ __launch_bounds__(256) void k_score_prepare(const ScoreParams p) {
    __shared__ float s_sh[8];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int f0 = p.pharm_ptr[g], nfg = min(p.pharm_ptr[g + 1] - f0, 64);
    const float a = p.alpha_tab[p.t_int], sg = p.sigma_tab[p.t_int];        // (the host entry has checked 0 <= t_int <= T)
    if (tid < 64) {
        float xc[3], xt[3], c1[3], c2[3];
        score_center(p, f0, nfg, tid, a, sg, xc, xt, c1, c2);
        if (tid < nfg) {
            const size_t f = (size_t)f0 + tid;
            const int row = 3 + p.nf;
            p.xn[p.Np + f] = make_float4(xt[0], xt[1], xt[2], 0.f);
            for (int k = 0; k < p.nf; ++k)
                p.pharm_h[f * p.nf + k] = __fadd_rn(__fmul_rn(a, p.h0[f * p.nf + k] / p.feat_norm), __fmul_rn(sg, p.noise[f * row + 3 + k]));
        }
        if (tid == 0) { s_sh[0] = c1[0]; s_sh[1] = c1[1]; s_sh[2] = c1[2]; s_sh[3] = c2[0]; s_sh[4] = c2[1]; s_sh[5] = c2[2]; }
    }
    __syncthreads();
    const float cx = s_sh[0], cy = s_sh[1], cz = s_sh[2], mx = s_sh[3], my = s_sh[4], mz = s_sh[5];
    for (int n = p.prot_ptr[g] + tid; n < p.prot_ptr[g + 1]; n += 256)
        p.xn[n] = make_float4(p.prot_x0[3 * (size_t)n] - cx - mx, p.prot_x0[3 * (size_t)n + 1] - cy - my, p.prot_x0[3 * (size_t)n + 2] - cz - mz, 0.f);
}

template <bool EPC, bool EPF>
__global__ __launch_bounds__(64) void k_score_eval(const ScoreParams p) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int f0 = p.pharm_ptr[g], nfg = min(p.pharm_ptr[g + 1] - f0, 64);
    const float a = p.alpha_tab[p.t_int], sg = p.sigma_tab[p.t_int];
    float xc[3], xt[3], c1[3], c2[3];
    score_center(p, f0, nfg, lane, a, sg, xc, xt, c1, c2);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < nfg) {
        const size_t f = (size_t)f0 + lane;
        const int row = 3 + p.nf;
        // every load of the center is requested before the first is used (pharm_nf <= 8)
        float ex[3], dx[3], eh[8], dh[8], ph[8], h0v[8];
#pragma unroll
        for (int c = 0; c < 3; ++c) { ex[c] = p.noise[f * row + c]; dx[c] = p.dyn_x[3 * f + c]; }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < p.nf) {
                const size_t o = f * p.nf + k;
                eh[k] = p.noise[f * row + 3 + k]; dh[k] = p.dyn_h[o]; ph[k] = p.pharm_h[o]; h0v[k] = p.h0[o];
            } else eh[k] = dh[k] = ph[k] = h0v[k] = 0.f;
        float xl = 0.f, err = 0.f;
        if constexpr (EPC) {
            // the prediction is the clean center in the frame before the second COM removal; the position error is the loss term
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = (dx[c] + c2[c]) - xc[c];
                xl += d * d;
            }
            err = xl;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = ex[c] - dx[c];
                xl += d * d;
                const float e = (xt[c] - sg * dx[c]) / a - xc[c];
                err += e * e;
            }
        }
        float hl = 0.f, bp = 0.f, bt = 0.f;
        int ip = 0, it = 0;
        if constexpr (EPF) {
            // cross-entropy of the logits against the clean type: first maxima like argmax, the row maximum taken off before expf
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < p.nf) {
                    if (k == 0 || dh[k] > bp) { bp = dh[k]; ip = k; }
                    if (k == 0 || h0v[k] > bt) { bt = h0v[k]; it = k; }
                }
            float se = 0.f, lt = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < p.nf) {
                    se += expf(dh[k] - bp);
                    if (k == it) lt = dh[k];
                }
            hl = logf(se) + bp - lt;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < p.nf) {
                    const float d = eh[k] - dh[k];
                    hl += d * d;
                    const float hp = (ph[k] - sg * dh[k]) / a, ht = h0v[k];
                    if (k == 0 || hp > bp) { bp = hp; ip = k; }                  // first maximum, like argmax
                    if (k == 0 || ht > bt) { bt = ht; it = k; }
                }
        }
        acc[0] = xl; acc[1] = hl; acc[2] = err; acc[3] = ip == it ? 1.0f : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = wave_sum(acc[q]);
    // lanes 0..3 store the four terms, lanes 0..1 the two score columns (in level order: the host enqueues the levels in order)
    const float mine = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : acc[3]));
    if (lane < 4 && p.terms) p.terms[(size_t)g * 4 + lane] = mine;
    if (lane < 2) {
        const float w = __fmul_rn(lane == 0 ? p.w_pos : p.w_feat, mine);
        float* dst = p.score + (size_t)g * 2 + lane;
        *dst = p.first ? w : __fadd_rn(*dst, w);
    }
}

}  // namespace

extern "C" {
void pfk_score_prepare(const ScoreParams* p, hipStream_t s) { hipLaunchKernelGGL(k_score_prepare, dim3(p->B), dim3(256), 0, s, *p); }
void pfk_score_eval(const ScoreParams* p, int ep_coord, int ep_feat, hipStream_t s) {
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(p->B), dim3(64), 0, s, *p); };
    if (ep_coord) { if (ep_feat) go(k_score_eval<true, true>); else go(k_score_eval<true, false>); }
    else { if (ep_feat) go(k_score_eval<false, true>); else go(k_score_eval<false, false>); }
}
}
