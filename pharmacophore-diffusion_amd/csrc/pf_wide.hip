// pf_wide.hip -- the width-generic inference family of libpfdyn (gfx950, fp32).
//
// One dynamics call (PharmRecDynamicsGVP.forward, dynamics_gvp.py:131-185) at the handle's widths: n_hidden_scalars S in
// 64..256 (multiples of 32), vector_size V in {16, 32}.  The tuned kernels of pf_kernels.hip / pf_rg.hip / pf_n16.hip are
// specialised to S = 128, V = 16; this family serves every other pair (and 128 / 16 under PFDYN_WIDE=1).  Launches:
//   k_wide_encode   the two encoders (every node)
//   k_wide_edge     per conv layer: the message chain of every edge slot of a tile list, all four etypes in one launch
//   k_wide_node     per conv layer: aggregation, norm, residual + GVPLayerNorm, the update chain, residual + GVPLayerNorm;
//                   the last layer's launch continues with the noise head of its centers
// The tile lists are the ones the specialised path uses (pf_set_pocket_batch): the last conv layer computes only the ff / pf
// messages and the centers, the layer before it only the active atoms (sources of pf edges), their "pa" in-edges and the
// centers.  A workgroup (four waves) owns PFW_ROWS rows; each row's message goes to its own slot row, and a node sums its
// in-edge rows in slot order -- no atomics, the same bits on every run.
// Scalar Linears: v_mfma_f32_16x16x4_f32, rows as the A operand from LDS, weights as the B operand streamed from L2 in the
// fragment order pf_host.cpp packs (pf_device.h: WideGvp).  The vector channel (K <= 33) runs on the vector ALU.
#include <hip/hip_runtime.h>
#include "pf_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float w_silu(float x) { return x / (1.0f + __expf(-x)); }
__device__ __forceinline__ float w_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

// LDS of one workgroup (floats): two scalar buffers [PFW_ROWS][ld], three vector buffers [PFW_ROWS][vs] (vs = 3 x channels),
// the gates [PFW_ROWS][V], and (node kernel) the residual rows [PFW_ROWS][S + 3 V]
struct WLay {
    float *sa, *sb, *va, *vb, *vh, *g, *sr;
    int ld, vs;
};
__host__ __device__ inline int wide_ld(int S, int V, bool edge) {
    const int k = S + (edge ? PF_R : 0) + V + (edge ? 1 : 0);       // widest to_feats_out input: [h, rbf, sh]
    return (k + 3) / 4 * 4 + 1;
}
__host__ __device__ inline int wide_vs(int V, bool edge) { return 3 * (V + (edge ? 1 : 0)); }
__host__ __device__ inline size_t wide_lds_floats(int S, int V, bool edge) {
    return (size_t)PFW_ROWS * (2 * wide_ld(S, V, edge) + 3 * wide_vs(V, edge) + V + (edge ? 0 : S + 3 * V)) + 2 * PFW_ROWS;
}
__device__ inline WLay wide_lay(float* base, int S, int V, bool edge) {
    WLay L;
    L.ld = wide_ld(S, V, edge); L.vs = wide_vs(V, edge);
    L.sa = base; L.sb = L.sa + PFW_ROWS * L.ld;
    L.va = L.sb + PFW_ROWS * L.ld; L.vb = L.va + PFW_ROWS * L.vs; L.vh = L.vb + PFW_ROWS * L.vs;
    L.g = L.vh + PFW_ROWS * L.vs;
    L.sr = L.g + PFW_ROWS * V;
    return L;
}

// out[r][n] = act(sum_k in[r][k] W[n][k] + b[n]) for the PFW_ROWS rows; in: LDS [PFW_ROWS][lda] with zeros in columns
// [K, 4 ceil(K / 4)); wp: fragment order (see pf_device.h).  act: 0 none, 1 SiLU, 2 sigmoid.  Wave w takes the output tiles
// w, w + 4, ... and both 16-row halves of the tile against each weight fragment.  The k-steps go in groups of four whose
// weight fragments are loaded one group ahead (the trip count is a run-time value: the compiler does not unroll the loop
// itself, and a load per k-step in front of its own two MFMAs serialises on the L2 latency).
__device__ void wide_linear(const float* in, int lda, int K, pf_gcf wp, pf_gcf bias, int N, float* out, int ldo, int act) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int KS = (K + 3) >> 2, NT = (N + 15) >> 4;
    const float* a0 = in + (lane & 15) * lda + (lane >> 4);
    const float* a1 = a0 + 16 * lda;
    for (int t = wave; t < NT; t += 4) {
        pf_gcf w = wp + (size_t)t * KS * 64 + lane;
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
        const int KS4 = KS & ~3;
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (KS4 > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = w[(size_t)j * 64];
        }
        for (int ks = 0; ks < KS4; ks += 4) {
            float nb[4] = {0.f, 0.f, 0.f, 0.f};
            if (ks + 4 < KS4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) nb[j] = w[(size_t)(ks + 4 + j) * 64];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * (ks + j)], b[j], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[4 * (ks + j)], b[j], c1, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = nb[j];
        }
        for (int ks = KS4; ks < KS; ++ks) {
            const float bk = w[(size_t)ks * 64];
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * ks], bk, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[4 * ks], bk, c1, 0, 0, 0);
        }
        const int col = 16 * t + (lane & 15);
        if (col < N) {
            const float bb = bias[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * (lane >> 4) + r;
                float x0 = c0[r] + bb, x1 = c1[r] + bb;
                if (act == 1) { x0 = w_silu(x0); x1 = w_silu(x1); }
                else if (act == 2) { x0 = w_sigmoid(x0); x1 = w_sigmoid(x1); }
                out[row * ldo + col] = x0;
                out[(row + 16) * ldo + col] = x1;
            }
        }
    }
}

// GVP.forward (gvp.py:89-116) on the PFW_ROWS rows: sin [.][ld] holds the si input scalars (its columns si .. get sh and the
// zero padding), vin [.][vs] the vi input channels; sout / vout receive so scalars and vo channels.  sig: sigmoid gates
// (identity otherwise: the noise head's last GVP).  Ends with a barrier.
__device__ void wide_gvp(const WideGvp* gp, float* sin, const float* vin, float* sout, float* vout, float* vh, float* g,
                         int ld, int vs, bool sig) {
    const WideGvp W = *gp;
    const int vi = W.vi, vo = W.vo, si = W.si, so = W.so, H = max(vi, vo);
    const int tid = threadIdx.x;
    // Vh = V^T Wh  [h][c]
    for (int i = tid; i < PFW_ROWS * H * 3; i += 256) {
        const int r = i / (H * 3), q = i - r * H * 3, hh = q / 3, c = q - hh * 3;
        const float* v = vin + r * vs + c;
        float acc = 0.f;
        for (int k = 0; k < vi; ++k) acc = fmaf(v[3 * k], W.wh[k * H + hh], acc);
        vh[r * vs + q] = acc;
    }
    __syncthreads();
    // sh = |Vh| (clamped), appended to the scalars; Vu = Vh^T Wu
    const int K = si + H, Kp = (K + 3) & ~3;
    for (int i = tid; i < PFW_ROWS * (Kp - si); i += 256) {
        const int r = i / (Kp - si), hh = i - r * (Kp - si);
        float x = 0.f;
        if (hh < H) {
            const float* p = vh + r * vs + 3 * hh;
            x = sqrtf(fmaxf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], 1e-8f));
        }
        sin[r * ld + si + hh] = x;
    }
    for (int i = tid; i < PFW_ROWS * vo * 3; i += 256) {
        const int r = i / (vo * 3), q = i - r * vo * 3, u = q / 3, c = q - u * 3;
        const float* p = vh + r * vs + c;
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(p[3 * k], W.wu[k * vo + u], acc);
        vout[r * vs + q] = acc;
    }
    __syncthreads();
    wide_linear(sin, ld, K, W.wm, W.bm, so, sout, ld, 1);
    __syncthreads();
    wide_linear(sout, ld, so, W.wg, W.bg, vo, g, vo, sig ? 2 : 0);
    __syncthreads();
    for (int i = tid; i < PFW_ROWS * vo * 3; i += 256) {
        const int r = i / (vo * 3), q = i - r * vo * 3;
        vout[r * vs + q] *= g[r * vo + q / 3];
    }
    __syncthreads();
}

// GVPLayerNorm (gvp.py:159-166) of the PFW_ROWS rows in place: eight lanes per row
__device__ void wide_layernorm(float* s, int ld, float* v, int vs, int S, int V, pf_gcf lw, pf_gcf lb) {
    const int r = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float* x = s + r * ld;
    float sum = 0.f;
    for (int f = sub; f < S; f += 8) sum += x[f];
    sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
    const float mean = sum / (float)S;
    float var = 0.f;
    for (int f = sub; f < S; f += 8) { const float c = x[f] - mean; var = fmaf(c, c, var); }
    var += __shfl_xor(var, 1); var += __shfl_xor(var, 2); var += __shfl_xor(var, 4);
    const float rstd = 1.0f / sqrtf(var / (float)S + 1e-5f);
    for (int f = sub; f < S; f += 8) x[f] = (x[f] - mean) * rstd * lw[f] + lb[f];
    float* y = v + r * vs;
    float vn = 0.f;
    for (int u = sub; u < V; u += 8) vn += fmaxf(y[3 * u] * y[3 * u] + y[3 * u + 1] * y[3 * u + 1] + y[3 * u + 2] * y[3 * u + 2], 1e-8f);
    vn += __shfl_xor(vn, 1); vn += __shfl_xor(vn, 2); vn += __shfl_xor(vn, 4);
    const float den = sqrtf(vn / (float)V + 1e-5f) + 1e-5f;
    for (int q = sub; q < 3 * V; q += 8) y[q] = y[q] / den;
}

__global__ __launch_bounds__(256) void k_wide_encode(const WideEncParams p) {
    // 32 lanes per node, eight nodes per workgroup
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), sub = threadIdx.x & 31;
    const int N = p.Np + p.Nf;
    if (row >= N) return;
    const int nt = row >= p.Np ? 1 : 0;
    const int nf = nt ? p.pharm_nf : p.rec_nf;
    const float* x = nt ? p.pharm_h + (size_t)(row - p.Np) * nf : p.prot_h0 + (size_t)row * nf;
    const float t = p.t ? p.t[p.gid[row]] : p.t_scalar;
    const int S = p.S;
    float y[PFW_MAXS / 32];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < PFW_MAXS / 32; ++i) {
        const int f = sub + 32 * i;
        y[i] = 0.f;
        if (f < S) {
            float acc = 0.f;
            for (int k = 0; k < nf; ++k) acc = fmaf(x[k], p.w[nt][(size_t)k * S + f], acc);
            acc = fmaf(t, p.w[nt][(size_t)nf * S + f], acc);
            y[i] = w_silu(acc + p.b[nt][f]);
            sum += y[i];
        }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)S;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < PFW_MAXS / 32; ++i)
        if (sub + 32 * i < S) { const float c = y[i] - mean; var = fmaf(c, c, var); }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) var += __shfl_xor(var, o);
    const float rstd = 1.0f / sqrtf(var / (float)S + 1e-5f);
#pragma unroll
    for (int i = 0; i < PFW_MAXS / 32; ++i) {
        const int f = sub + 32 * i;
        if (f < S) p.h_out[(size_t)row * S + f] = (y[i] - mean) * rstd * p.ln_w[nt][f] + p.ln_b[nt][f];
    }
}

__global__ __launch_bounds__(256) void k_wide_edge(const WideEdgeParams p) {
    extern __shared__ float lds[];
    const EdgeTile t = p.tiles[blockIdx.x];
    int nvalid = t.n;
    if (t.cnt_idx >= 0) nvalid = min(nvalid, max(p.dyn_cnt[t.cnt_idx] - t.rel, 0));
    if (nvalid <= 0) return;
    const int S = p.S, V = p.V, tid = threadIdx.x;
    WLay L = wide_lay(lds, S, V, true);
    int* src = reinterpret_cast<int*>(L.sr);             // (the edge kernel has no residual rows)
    // geometry (gvp.py:474-480, 545-547): channel 0 = unit displacement, scalars [h_src, rbf(d)]
    if (tid < PFW_ROWS) {
        const int e = t.e0 + min(tid, nvalid - 1);        // idle rows shadow the last valid slot
        const int s = p.esrc[e], d = p.edst[e];
        src[tid] = s;
        const float4 xs = p.xn[s], xd = p.xn[d];
        const float dx = xs.x - xd.x, dy = xs.y - xd.y, dz = xs.z - xd.z;
        const float dist = sqrtf(fmaxf((dx * dx + dy * dy) + dz * dz, 1e-8f)) + 1e-8f;
        float* v0 = L.va + tid * L.vs;
        v0[0] = dx / dist; v0[1] = dy / dist; v0[2] = dz / dist;
        float* sr = L.sa + tid * L.ld + S;
#pragma unroll
        for (int k = 0; k < PF_R; ++k) {
            const float z = (dist - p.rbf_mu[k]) / p.rbf_sigma;
            sr[k] = __expf(-(z * z));
        }
    }
    __syncthreads();
    for (int i = tid; i < PFW_ROWS * S; i += 256) {
        const int r = i / S, f = i - r * S;
        L.sa[r * L.ld + f] = p.h[(size_t)src[r] * S + f];
    }
    for (int i = tid; i < PFW_ROWS * 3 * V; i += 256) {
        const int r = i / (3 * V), q = i - r * 3 * V;
        L.va[r * L.vs + 3 + q] = p.layer0 ? 0.f : p.v[(size_t)src[r] * 3 * V + q];
    }
    __syncthreads();
    const WideGvp* w = p.w + (size_t)t.et * p.n_gvps;
    float *si = L.sa, *so = L.sb, *vi = L.va, *vo = L.vb;
    for (int j = 0; j < p.n_gvps; ++j) {
        wide_gvp(w + j, si, vi, so, vo, L.vh, L.g, L.ld, L.vs, true);
        float* x = si; si = so; so = x;
        x = vi; vi = vo; vo = x;
    }
    for (int i = tid; i < nvalid * S; i += 256) {
        const int r = i / S, f = i - r * S;
        p.msg_s[(size_t)(t.e0 + r) * S + f] = si[r * L.ld + f];
    }
    for (int i = tid; i < nvalid * 3 * V; i += 256) {
        const int r = i / (3 * V), q = i - r * 3 * V;
        p.msg_v[(size_t)(t.e0 + r) * 3 * V + q] = vi[r * L.vs + q];
    }
}

__global__ __launch_bounds__(256) void k_wide_node(const WideNodeParams p) {
    extern __shared__ float lds[];
    const NodeTile t = p.tiles[blockIdx.x];
    int tn = t.n;
    if (t.cnt_idx >= 0) tn = min(tn, max(p.dyn_cnt[t.cnt_idx] - t.rel, 0));
    if (tn <= 0) return;
    const int S = p.S, V = p.V, V3 = 3 * V, tid = threadIdx.x, nt = t.ntype;
    WLay L = wide_lay(lds, S, V, false);
    float* vr = L.sr + PFW_ROWS * S;
    int* node = reinterpret_cast<int*>(vr + PFW_ROWS * V3);
    float* inv = reinterpret_cast<float*>(node + PFW_ROWS);
    if (tid < PFW_ROWS) {
        const int j = min(tid, tn - 1);
        const int n = t.ids ? p.row_ids[t.n0 + j] : t.n0 + j;
        node[tid] = n;
        float nv = 1.0f;                                       // gvp.py:504-512
        if (p.norm_mode == 1) nv = p.norm_value;
        else if (p.norm_mode == 2) nv = p.gnorm[nt * p.B + p.gid[n]];
        inv[tid] = nv;
    }
    __syncthreads();
    // per etype sum (or mean) of the in-edge rows in slot order, the cross-type sum, the norm, the residual
    const int slot1 = nt == 0 ? p.pp_slot : 1;
    for (int i = tid; i < PFW_ROWS * (S + V3); i += 256) {
        const int r = i / (S + V3), q = i - r * (S + V3);
        const int n = node[r];
        const bool sc = q < S;
        const float* m = sc ? p.msg_s + q : p.msg_v + (q - S);
        const int ld = sc ? S : V3;
        float agg = 0.f;
        for (int k = 0; k < 2; ++k) {
            const int slot = k == 0 ? 0 : slot1;
            const int st = p.in_start[slot * p.N + n], c = p.in_cnt[slot * p.N + n];
            float a = 0.f;
            for (int e = st; e < st + c; ++e) a += m[(size_t)e * ld];
            if (p.norm_mode == 0 && c > 0) a = a / (float)c;
            agg = k == 0 ? a : agg + a;
        }
        agg = agg / inv[r];
        if (sc) L.sa[r * L.ld + q] = p.h_in[(size_t)n * S + q] + agg;
        else L.va[r * V3 + (q - S)] = (p.layer0 ? 0.f : p.v_in[(size_t)n * V3 + (q - S)]) + agg;
    }
    __syncthreads();
    wide_layernorm(L.sa, L.ld, L.va, V3, S, V, p.ln1_w[nt], p.ln1_b[nt]);
    __syncthreads();
    for (int i = tid; i < PFW_ROWS * S; i += 256) L.sr[i] = L.sa[(i / S) * L.ld + i % S];
    for (int i = tid; i < PFW_ROWS * V3; i += 256) vr[i] = L.va[i];
    __syncthreads();
    float *si = L.sa, *so = L.sb, *vi = L.va, *vo = L.vb;
    for (int j = 0; j < p.n_upd; ++j) {
        wide_gvp(p.upd[nt] + j, si, vi, so, vo, L.vh, L.g, L.ld, V3, true);
        float* x = si; si = so; so = x;
        x = vi; vi = vo; vo = x;
    }
    for (int i = tid; i < PFW_ROWS * S; i += 256) { const int r = i / S, f = i - r * S; si[r * L.ld + f] += L.sr[i]; }
    for (int i = tid; i < PFW_ROWS * V3; i += 256) vi[i] += vr[i];
    __syncthreads();
    wide_layernorm(si, L.ld, vi, V3, S, V, p.ln2_w[nt], p.ln2_b[nt]);
    __syncthreads();
    if (p.head == nullptr) {
        for (int i = tid; i < tn * S; i += 256) { const int r = i / S, f = i - r * S; p.h_out[(size_t)node[r] * S + f] = si[r * L.ld + f]; }
        for (int i = tid; i < tn * V3; i += 256) { const int r = i / V3, q = i - r * V3; p.v_out[(size_t)node[r] * V3 + q] = vi[r * V3 + q]; }
        return;
    }
    // noise head (dynamics_gvp.py:37-42): GVP chain, the last one (V -> 1 channel, S -> 64 scalars) ungated, to_scalar_output
    for (int j = 0; j < p.n_head; ++j) {
        wide_gvp(p.head + j, si, vi, so, vo, L.vh, L.g, L.ld, V3, j != p.n_head - 1);
        float* x = si; si = so; so = x;
        x = vi; vi = vo; vo = x;
    }
    for (int i = tid; i < tn * p.pharm_nf; i += 256) {
        const int r = i / p.pharm_nf, k = i - r * p.pharm_nf;
        const float* x = si + r * L.ld;
        float acc = 0.f;
        for (int f = 0; f < 64; ++f) acc = fmaf(x[f], p.w_out[k * 64 + f], acc);
        p.eps_h[(size_t)(node[r] - p.node_base) * p.pharm_nf + k] = acc + p.b_out[k];
    }
    for (int i = tid; i < tn * 3; i += 256) {
        const int r = i / 3, c = i - r * 3;
        p.eps_x[(size_t)(node[r] - p.node_base) * 3 + c] = vi[r * V3 + c];
    }
}

}  // namespace

extern "C" {
size_t pfk_wide_lds_bytes(int S, int V, int edge) { return wide_lds_floats(S, V, edge != 0) * sizeof(float); }

void pfk_wide_encode(const WideEncParams* p, hipStream_t s) {
    const int N = p->Np + p->Nf;
    if (N == 0) return;
    hipLaunchKernelGGL(k_wide_encode, dim3((N + 7) / 8), dim3(256), 0, s, *p);
}
void pfk_wide_edge(const WideEdgeParams* p, hipStream_t s) {
    if (p->ntiles == 0) return;
    const size_t bytes = pfk_wide_lds_bytes(p->S, p->V, 1);
    // (up to 160 KB of LDS per workgroup, set by the widths: the limit is raised on the current device before every launch)
    (void)hipFuncSetAttribute((const void*)k_wide_edge, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    hipLaunchKernelGGL(k_wide_edge, dim3(p->ntiles), dim3(256), bytes, s, *p);
}
void pfk_wide_node(const WideNodeParams* p, hipStream_t s) {
    if (p->ntiles == 0) return;
    const size_t bytes = pfk_wide_lds_bytes(p->S, p->V, 0);
    (void)hipFuncSetAttribute((const void*)k_wide_node, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    hipLaunchKernelGGL(k_wide_node, dim3(p->ntiles), dim3(256), bytes, s, *p);
}
}
