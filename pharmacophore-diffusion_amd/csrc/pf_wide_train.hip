// pf_wide_train.hip -- the gradient kernels of the width-generic family of libpfdyn (gfx950, fp32).
//
// The reverse of run_dynamics_wide at the handle's widths (n_hidden_scalars S in 64..256, vector_size V in {16, 32}), behind the
// training form of the forward kernels (pf_wide.hip: k_wide_edge<true>, k_wide_node<true>), which kept per conv layer the input
// rows of every chain level (message chains per edge slot, update chains per node), the rows in front of both GVPLayerNorms, and
// for the centers the head's level inputs and its 64 output scalars.  Launches of one backward pass:
//   k_wt_head_out   to_scalar_output and the vector output of the head
//   k_wt_chain      one GVP level of every chain of a tile list; per conv layer from last to first: the head levels (last layer
//                   only), the update-chain levels, the message-chain levels -- each level a launch, last level first
//   k_wt_norm       a GVPLayerNorm with the GVPDropout beside it: "post" (LayerNorm 2, residual dropout) in front of the update
//                   chain's backward, "pre" (LayerNorm 1, message dropout, the message norm) behind it
//   k_wt_encode     the two encoders (and, when asked for, dL/d(the centers' feature rows))
//   k_wt_center_sum only when dL/d(center coordinates) is asked for: the level-0 launches of the message chains then also leave
//                   dL/d(x_src - x_dst) per edge slot (wt_edge_geometry), and this launch sums every center's rows in a fixed order
//   k_wt_reduce     the workgroups' gradient copies summed in index order: every element of the gradient vector is stored
// A level is recomputed from its kept input (Vh, sh, z, a, the gates), then differentiated:
//   dgate = sum_c dVout Vu, dVu = dVout gate, dpre = dgate gate', dWg += dpre (x) a, da = dA + Wg^T dpre, dz = da SiLU'(z),
//   dWm += dz (x) [s, sh], d[s, sh] = Wm^T dz, dVh = Wu dVu + dsh Vh / sh, dWu += Vh^T dVu, dWh += V^T dVh, dV = Wh dVh
// Scalar products run on v_mfma_f32_16x16x4_f32 (exact fp32): the 16 rows of a sub-tile are the A operand of the forward
// Linears and of Wm^T dz (whose B operand is to_feats_out as stored, 16 consecutive floats per k-row), and the K dimension of the
// weight gradients dz^T [s, sh] and dpre^T a.  The vector-channel products (K <= 33) run on the vector ALU.
// Rows of a sub-tile past the tile's valid ones carry a zero upstream gradient and zero inputs: they add nothing anywhere.
// No float atomics: weight gradients go to per-workgroup copies (pf_train.h), the scatter of dL/d(h_src, v_src) to the source
// nodes to 64-bit fixed-point accumulators (pfk_fix_scale / pfk_fix_apply of pf_train.hip) -- the same bits on every run.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "pf_device.h"
#include "pf_train.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int R = PFWT_ROWS;

__device__ __forceinline__ float t_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }

__device__ __forceinline__ float wt_drop(const WtCommon& c, uint32_t stream, int n, int col) {
    const uint32_t elem = (uint32_t)n * (uint32_t)(c.S + c.V) + (uint32_t)col;
    if (c.mask_override) return c.mask_override[(size_t)stream * c.N * (c.S + c.V) + elem];
    if (c.drop_thr == 0u) return 1.0f;
    return pf_drop_hash(c.seed, stream, elem) < c.drop_thr ? 0.0f : c.drop_scale;
}

// out[r][n] = sum_k in[r][k] W[n][k] + b[n] for the R rows; in: LDS [R][lda] with zeros in columns [K, 4 ceil(K / 4)); W: row-major
// [N][K] in the flat parameter vector.  Wave w takes the output tiles w, w + 4, ...
__device__ void wt_lin(const float* in, int lda, int K, const float* W, const float* b, int N, float* out, int ldo) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int KS = (K + 3) >> 2, NT = (N + 15) >> 4;
    const float* a0 = in + (lane & 15) * lda + (lane >> 4);
    for (int t = wave; t < NT; t += 4) {
        const int n = 16 * t + (lane & 15);
        const float* w = W + (size_t)min(n, N - 1) * K;
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < KS; ++ks) {
            const int k = 4 * ks + (lane >> 4);
            float bv = 0.f;
            if (n < N && k < K) bv = w[k];
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * ks], bv, c, 0, 0, 0);
        }
        if (n < N) {
            const float bb = b[n];
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(4 * (lane >> 4) + r) * ldo + n] = c[r] + bb;
        }
    }
}

// out[r][n] = sum_k in[r][k] W[k][n] for the R rows; W: row-major [K][N] in the flat parameter vector, K a multiple of 4
__device__ void wt_lin_t(const float* in, int lda, int K, const float* W, int N, float* out, int ldo) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int KS = K >> 2, NT = (N + 15) >> 4;
    const float* a0 = in + (lane & 15) * lda + (lane >> 4);
    for (int t = wave; t < NT; t += 4) {
        const int n = 16 * t + (lane & 15);
        const float* w = W + (size_t)(lane >> 4) * N + min(n, N - 1);
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < KS; ++ks) {
            float bv = 0.f;
            if (n < N) bv = w[(size_t)4 * ks * N];
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[4 * ks], bv, c, 0, 0, 0);
        }
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(4 * (lane >> 4) + r) * ldo + n] = c[r];
        }
    }
}

// dst[m][n] += sum_r X[r][m] Y[r][n] over the R rows (the K dimension: four k-steps); dst: row-major [M][N] in this workgroup's
// gradient copy.  Every element of dst belongs to one lane of one wave.
__device__ void wt_outer(const float* X, int ldx, int M, const float* Y, int ldy, int N, float* dst) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int MT = (M + 15) >> 4, NT = (N + 15) >> 4;
    for (int t = wave; t < MT * NT; t += 4) {
        const int mt = t / NT, nt = t - mt * NT;
        const int m = 16 * mt + (lane & 15), n = 16 * nt + (lane & 15);
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < R / 4; ++ks) {
            const int r = 4 * ks + (lane >> 4);
            float av = 0.f, bv = 0.f;
            if (m < M) av = X[r * ldx + m];
            if (n < N) bv = Y[r * ldy + n];
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mm = 16 * mt + 4 * (lane >> 4) + r;
            if (mm < M && n < N) dst[(size_t)mm * N + n] += c[r];
        }
    }
}

// LDS of k_wt_chain (floats per row): the level's scalar input with sh behind it [ld] (later dL/d of both), z (later dz), a,
// the upstream dA [lz each]; V, Vh, Vu, dVout (later dVu, then dV), dVh [vs each]; the gates and dpre [gw each]
struct WtLay { int ld, lz, vs, gw; };
__host__ __device__ inline WtLay wt_lay(int S, int V, bool edge) {
    WtLay L;
    const int K = S + (edge ? PF_R : 0) + V + (edge ? 1 : 0);
    L.ld = (K + 3) / 4 * 4 + 1; L.lz = S + 1; L.vs = 3 * (V + (edge ? 1 : 0)); L.gw = V + (edge ? 1 : 0);
    return L;
}
__host__ __device__ inline size_t wt_chain_lds_floats(int S, int V, bool edge) {
    const WtLay L = wt_lay(S, V, edge);
    return (size_t)R * (L.ld + 3 * L.lz + 5 * L.vs + 2 * L.gw) + 4 * R;
}

// The edge geometry's backward (gvp.py:474-480, _rbf :26-41, _norm_no_nan :12-19) for one edge row of a level-0 message chain:
// diff = x_src - x_dst, n2 = |diff|^2, d = sqrt(max(n2, 1e-8)) + 1e-8, u = diff / d, rbf_k = exp(-((d - mu_k) / sigma)^2); given
// g_rbf [PF_R] and g_u [3],
//   g_d = sum_k g_rbf[k] rbf_k (-2 (d - mu_k) / sigma^2) - (g_u . diff) / d^2,  g_diff = g_u / d + (n2 > 1e-8 ? g_d diff / sqrt(n2) : 0)
// (nothing through the clamped norm).  diff, n2 and d in k_wide_edge's arithmetic, so the clamp decides as the forward's did; the
// rbf values as the forward kept them; the few sums of a row in fp64, rounded once.
__device__ __forceinline__ void wt_edge_geometry(const WtChainParams& p, int s, int d, int slot, const float* g_rbf, const float* g_u) {
    const float4 xs = p.xn[s], xd = p.xn[d];
    const float dx = xs.x - xd.x, dy = xs.y - xd.y, dz = xs.z - xd.z;
    const float n2 = (dx * dx + dy * dy) + dz * dz;
    const float dist = sqrtf(fmaxf(n2, 1e-8f)) + 1e-8f;
    const float* rbf = p.sv_s + (size_t)(slot - p.sv_base) * p.sv_ls + p.c.S;
    const double dd = (double)dist, sg = (double)p.rbf_sigma;
    double gd = 0.0;
#pragma unroll
    for (int k = 0; k < PF_R; ++k) gd += (double)g_rbf[k] * (double)rbf[k] * (-2.0 * (dd - (double)p.rbf_mu[k]) / (sg * sg));
    gd -= ((double)g_u[0] * dx + (double)g_u[1] * dy + (double)g_u[2] * dz) / (dd * dd);
    const double m = n2 > 1e-8f ? gd / sqrt((double)n2) : 0.0;
    float* o = p.g_diff + (size_t)slot * 3;
    o[0] = (float)((double)g_u[0] / dd + m * dx);
    o[1] = (float)((double)g_u[1] / dd + m * dy);
    o[2] = (float)((double)g_u[2] / dd + m * dz);
}

// WG: the weight-gradient products (the full pass).  Without it (the inputs-only pass: pf_dynamics_input_vjp, a guided step) the
// kernel forms no pointer into the gradient copies and skips every dW product; dL/d(input) takes the same operations either way
template <bool EDGE, bool WG>
__global__ __launch_bounds__(256) void k_wt_chain(const WtChainParams p) {
    extern __shared__ float lds[];
    const int S = p.c.S, V = p.c.V, tid = threadIdx.x;
    const WtLay L = wt_lay(S, V, EDGE);
    const int ld = L.ld, lz = L.lz, vs = L.vs, gw = L.gw;
    float* in = lds;
    float* z = in + R * ld;
    float* a = z + R * lz;
    float* da = a + R * lz;
    float* vin = da + R * lz;
    float* vh = vin + R * vs;
    float* vu = vh + R * vs;
    float* dv = vu + R * vs;
    float* dvh = dv + R * vs;
    float* gate = dvh + R * vs;
    float* dpre = gate + R * gw;
    int* rid = reinterpret_cast<int*>(dpre + R * gw);
    int* src = rid + R;
    int* dst = src + R;
    float* sc = reinterpret_cast<float*>(dst + R);
    float* gp = nullptr;
    if constexpr (WG) gp = p.c.gpart + (size_t)blockIdx.x * p.c.gstride;
    const float* W = p.c.W;
    for (int ti = blockIdx.x; ti < p.n_tiles; ti += gridDim.x) {
        int nvalid, ty, e0 = 0, n0 = 0, ids = 0;
        if constexpr (EDGE) {
            const EdgeTile t = p.etiles[ti];
            nvalid = t.n;
            if (t.cnt_idx >= 0) nvalid = min(nvalid, max(p.dyn_cnt[t.cnt_idx] - t.rel, 0));
            ty = t.et; e0 = t.e0;
        } else {
            const NodeTile t = p.ntiles[ti];
            nvalid = t.n;
            if (t.cnt_idx >= 0) nvalid = min(nvalid, max(p.dyn_cnt[t.cnt_idx] - t.rel, 0));
            ty = t.ntype; n0 = t.n0; ids = t.ids;
        }
        const GvpT G = p.g[ty * p.g_stride + p.level];
        const int vi = G.vi, vo = G.vo, si = G.si, so = G.so, H = G.h, K = si + H, Kp = (K + 3) & ~3;
        const bool agg_up = EDGE && p.last;
        for (int r0 = 0; r0 < nvalid; r0 += R) {
            const int nv = min(R, nvalid - r0);
            __syncthreads();
            if (tid < R) {
                int id = 0, s_ = 0, d_ = 0;
                float scale = 0.f;
                if (tid < nv) {
                    if constexpr (EDGE) {
                        id = e0 + r0 + tid;
                        s_ = p.esrc[id]; d_ = p.edst[id];
                        scale = 1.0f;
                        if (p.norm_mode == 0) {          // fn.mean over the etype's in-edges (gvp.py:488-497)
                            const int slot = (ty == ET_FF || ty == ET_FP) ? 0 : (ty == ET_PP ? p.pp_slot : 1);
                            const int cnt = p.in_cnt[slot * p.c.N + d_];
                            scale = cnt > 0 ? 1.0f / (float)cnt : 0.f;
                        }
                    } else {
                        id = ids ? p.row_ids[n0 + r0 + tid] : n0 + r0 + tid;
                    }
                }
                rid[tid] = id; src[tid] = s_; dst[tid] = d_; sc[tid] = scale;
            }
            __syncthreads();
            // the level's input and the upstream gradient; rows past nv: zeros
            for (int i = tid; i < R * Kp; i += 256) {
                const int r = i / Kp, f = i - r * Kp;
                float x = 0.f;
                if (r < nv && f < si) x = p.sv_s[(size_t)(rid[r] - p.sv_base) * p.sv_ls + f];
                in[r * ld + f] = x;
            }
            for (int i = tid; i < R * vi * 3; i += 256) {
                const int r = i / (vi * 3), q = i - r * vi * 3;
                vin[r * vs + q] = r < nv ? p.sv_v[(size_t)(rid[r] - p.sv_base) * p.sv_lv + q] : 0.f;
            }
            for (int i = tid; i < R * so; i += 256) {
                const int r = i / so, f = i - r * so;
                float x = 0.f;
                if (r < nv) x = agg_up ? p.gagg_s[(size_t)dst[r] * S + f] * sc[r] : p.up_s[(size_t)rid[r] * p.up_ls + f];
                da[r * lz + f] = x;
            }
            for (int i = tid; i < R * vo * 3; i += 256) {
                const int r = i / (vo * 3), q = i - r * vo * 3;
                float x = 0.f;
                if (r < nv) x = agg_up ? p.gagg_v[(size_t)dst[r] * 3 * V + q] * sc[r] : p.up_v[(size_t)rid[r] * p.up_lv + q];
                dv[r * vs + q] = x;
            }
            __syncthreads();
            // the level once more (wide_gvp's order): Vh, sh, Vu, z, a, the gates
            for (int i = tid; i < R * H * 3; i += 256) {
                const int r = i / (H * 3), q = i - r * H * 3, hh = q / 3, c = q - hh * 3;
                const float* v = vin + r * vs + c;
                float acc = 0.f;
                for (int k = 0; k < vi; ++k) acc = fmaf(v[3 * k], W[G.o_Wh + k * H + hh], acc);
                vh[r * vs + q] = acc;
            }
            __syncthreads();
            for (int i = tid; i < R * (Kp - si); i += 256) {
                const int r = i / (Kp - si), hh = i - r * (Kp - si);
                float x = 0.f;
                if (hh < H) {
                    const float* q = vh + r * vs + 3 * hh;
                    x = sqrtf(fmaxf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2], 1e-8f));
                }
                in[r * ld + si + hh] = x;
            }
            for (int i = tid; i < R * vo * 3; i += 256) {
                const int r = i / (vo * 3), q = i - r * vo * 3, u = q / 3, c = q - u * 3;
                const float* v = vh + r * vs + c;
                float acc = 0.f;
                for (int k = 0; k < H; ++k) acc = fmaf(v[3 * k], W[G.o_Wu + k * vo + u], acc);
                vu[r * vs + q] = acc;
            }
            __syncthreads();
            wt_lin(in, ld, K, W + G.o_Wm, W + G.o_bm, so, z, lz);
            __syncthreads();
            for (int i = tid; i < R * so; i += 256) {
                const int r = i / so, f = i - r * so;
                const float zz = z[r * lz + f];
                a[r * lz + f] = zz * t_sigmoid(zz);
            }
            __syncthreads();
            wt_lin(a, lz, so, W + G.o_Wg, W + G.o_bg, vo, gate, gw);
            __syncthreads();
            // dgate, dpre, dVu
            for (int i = tid; i < R * vo; i += 256) {
                const int r = i / vo, u = i - r * vo;
                const float pre = gate[r * gw + u];
                const float g = G.sig ? t_sigmoid(pre) : pre;
                float* d = dv + r * vs + 3 * u;
                const float* v = vu + r * vs + 3 * u;
                const float dg = d[0] * v[0] + d[1] * v[1] + d[2] * v[2];
                dpre[r * gw + u] = G.sig ? dg * g * (1.0f - g) : dg;
                d[0] *= g; d[1] *= g; d[2] *= g;
            }
            __syncthreads();
            if constexpr (WG) {
                wt_outer(dpre, gw, vo, a, lz, so, gp + G.o_Wg);
                if (tid < vo) {
                    float s = 0.f;
                    for (int r = 0; r < R; ++r) s += dpre[r * gw + tid];
                    gp[G.o_bg + tid] += s;
                }
                __syncthreads();
            }
            // da = dA + Wg^T dpre, dz = da SiLU'(z) (into z)
            for (int i = tid; i < R * so; i += 256) {
                const int r = i / so, f = i - r * so;
                float acc = da[r * lz + f];
                for (int c = 0; c < vo; ++c) acc = fmaf(W[G.o_Wg + c * so + f], dpre[r * gw + c], acc);
                const float zz = z[r * lz + f], s = t_sigmoid(zz);
                z[r * lz + f] = acc * s * (1.0f + zz * (1.0f - s));
            }
            __syncthreads();
            if constexpr (WG) {
                wt_outer(z, lz, so, in, ld, K, gp + G.o_Wm);
                for (int f = tid; f < so; f += 256) {
                    float s = 0.f;
                    for (int r = 0; r < R; ++r) s += z[r * lz + f];
                    gp[G.o_bm + f] += s;
                }
                __syncthreads();
            }
            wt_lin_t(z, lz, so, W + G.o_Wm, K, in, ld);          // d[s, sh] over the input
            __syncthreads();
            // dVh = Wu dVu + dsh Vh / sh (nothing through a clamped norm)
            for (int i = tid; i < R * H * 3; i += 256) {
                const int r = i / (H * 3), q = i - r * H * 3, hh = q / 3, c = q - hh * 3;
                const float* d = dv + r * vs + c;
                float acc = 0.f;
                for (int u = 0; u < vo; ++u) acc = fmaf(W[G.o_Wu + hh * vo + u], d[3 * u], acc);
                const float* x = vh + r * vs + 3 * hh;
                const float n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
                if (n2 > 1e-8f) acc += in[r * ld + si + hh] * x[c] / sqrtf(n2);
                dvh[r * vs + q] = acc;
            }
            __syncthreads();
            if constexpr (WG) {
                for (int i = tid; i < H * vo; i += 256) {
                    const int k = i / vo, u = i - k * vo;
                    float s = 0.f;
                    for (int r = 0; r < R; ++r) {
                        const float* x = vh + r * vs + 3 * k;
                        const float* d = dv + r * vs + 3 * u;
                        s += x[0] * d[0] + x[1] * d[1] + x[2] * d[2];
                    }
                    gp[G.o_Wu + i] += s;
                }
                for (int i = tid; i < vi * H; i += 256) {
                    const int k = i / H, hh = i - k * H;
                    float s = 0.f;
                    for (int r = 0; r < R; ++r) {
                        const float* x = vin + r * vs + 3 * k;
                        const float* d = dvh + r * vs + 3 * hh;
                        s += x[0] * d[0] + x[1] * d[1] + x[2] * d[2];
                    }
                    gp[G.o_Wh + i] += s;
                }
                __syncthreads();
            }
            for (int i = tid; i < R * vi * 3; i += 256) {       // dV = Wh dVh (over dVu)
                const int r = i / (vi * 3), q = i - r * vi * 3, k = q / 3, c = q - k * 3;
                const float* d = dvh + r * vs + c;
                float acc = 0.f;
                for (int hh = 0; hh < H; ++hh) acc = fmaf(W[G.o_Wh + k * H + hh], d[3 * hh], acc);
                dv[r * vs + q] = acc;
            }
            __syncthreads();
            if (EDGE && p.level == 0) {
                // dL/d(h_src, v_src) to the source nodes; the rbf columns and the displacement channel are constants
                const float fs = p.fix[0];
                for (int i = tid; i < nv * S; i += 256) {
                    const int r = i / S, f = i - r * S;
                    atomicAdd(reinterpret_cast<unsigned long long*>(p.A_h + (size_t)src[r] * S + f),
                              (unsigned long long)__float2ll_rn(in[r * ld + f] * fs));
                }
                if (!p.l0)
                    for (int i = tid; i < nv * 3 * V; i += 256) {
                        const int r = i / (3 * V), q = i - r * 3 * V;
                        atomicAdd(reinterpret_cast<unsigned long long*>(p.A_v + (size_t)src[r] * 3 * V + q),
                                  (unsigned long long)__float2ll_rn(dv[r * vs + 3 + q] * fs));
                    }
                if (p.g_diff && ty != ET_PP && tid < nv) wt_edge_geometry(p, src[tid], dst[tid], rid[tid], in + tid * ld + S, dv + tid * vs);
            } else {
                for (int i = tid; i < nv * si; i += 256) {
                    const int r = i / si, f = i - r * si;
                    p.out_s[(size_t)rid[r] * p.out_ls + f] = in[r * ld + f];
                }
                for (int i = tid; i < nv * vi * 3; i += 256) {
                    const int r = i / (vi * 3), q = i - r * vi * 3;
                    p.out_v[(size_t)rid[r] * p.out_lv + q] = dv[r * vs + q];
                }
            }
        }
    }
}

// GVPLayerNorm (gvp.py:159-166, wide_layernorm's arithmetic) backward for the rows of a node tile list, eight lanes per row
template <bool WG>
__global__ __launch_bounds__(256) void k_wt_norm(const WtNormParams p) {
    __shared__ float s_mean[PFW_ROWS], s_rstd[PFW_ROWS];
    __shared__ int s_node[PFW_ROWS];
    const int S = p.c.S, V = p.c.V, V3 = 3 * V, tid = threadIdx.x;
    float* gp = nullptr;
    if constexpr (WG) gp = p.c.gpart + (size_t)blockIdx.x * p.c.gstride;
    const float* W = p.c.W;
    for (int ti = blockIdx.x; ti < p.n_tiles; ti += gridDim.x) {
        const NodeTile t = p.tiles[ti];
        int tn = t.n;
        if (t.cnt_idx >= 0) tn = min(tn, max(p.dyn_cnt[t.cnt_idx] - t.rel, 0));
        if (tn <= 0) continue;
        const int nt = t.ntype;
        const int r = tid >> 3, sub = tid & 7;
        const bool live = r < tn;
        const int j = min(r, tn - 1);
        const int n = t.ids ? p.row_ids[t.n0 + j] : t.n0 + j;
        float mul = 1.0f;
        if (p.use_norm) {
            float nv = 1.0f;
            if (p.norm_mode == 1) nv = p.norm_value;
            else if (p.norm_mode == 2) nv = p.gnorm[nt * p.B + p.gid[n]];
            mul = 1.0f / nv;
        }
        const float* x = p.x_s + (size_t)n * S;
        const float* dA = p.dyA_s + (size_t)n * S;
        const float* dB = p.dyB_s ? p.dyB_s + (size_t)n * S : nullptr;
        const float* lw = W + p.o_lw[nt];
        float sum = 0.f;
        for (int f = sub; f < S; f += 8) sum += x[f];
        sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
        const float mean = sum / (float)S;
        float var = 0.f;
        for (int f = sub; f < S; f += 8) { const float c = x[f] - mean; var = fmaf(c, c, var); }
        var += __shfl_xor(var, 1); var += __shfl_xor(var, 2); var += __shfl_xor(var, 4);
        const float rstd = 1.0f / sqrtf(var / (float)S + 1e-5f);
        float m1 = 0.f, m2 = 0.f;
        for (int f = sub; f < S; f += 8) {
            const float g = (dA[f] + (dB ? dB[f] : 0.f)) * lw[f];
            m1 += g; m2 = fmaf(g, (x[f] - mean) * rstd, m2);
        }
        m1 += __shfl_xor(m1, 1); m1 += __shfl_xor(m1, 2); m1 += __shfl_xor(m1, 4);
        m2 += __shfl_xor(m2, 1); m2 += __shfl_xor(m2, 2); m2 += __shfl_xor(m2, 4);
        m1 /= (float)S; m2 /= (float)S;
        if (live)
            for (int f = sub; f < S; f += 8) {
                const float g = (dA[f] + (dB ? dB[f] : 0.f)) * lw[f];
                const float dx = rstd * (g - m1 - (x[f] - mean) * rstd * m2);
                p.out1_s[(size_t)n * S + f] = dx;
                p.out2_s[(size_t)n * S + f] = dx * wt_drop(p.c, (uint32_t)p.stream, n, f) * mul;
            }
        // vectors: y = v / den, den = sqrt(mean_u max(|v_u|^2, 1e-8) + 1e-5) + 1e-5
        const float* y = p.x_v + (size_t)n * V3;
        const float* eA = p.dyA_v + (size_t)n * V3;
        const float* eB = p.dyB_v ? p.dyB_v + (size_t)n * V3 : nullptr;
        float vn = 0.f, dot = 0.f;
        for (int u = sub; u < V; u += 8) {
            vn += fmaxf(y[3 * u] * y[3 * u] + y[3 * u + 1] * y[3 * u + 1] + y[3 * u + 2] * y[3 * u + 2], 1e-8f);
            for (int c = 0; c < 3; ++c) dot = fmaf(eA[3 * u + c] + (eB ? eB[3 * u + c] : 0.f), y[3 * u + c], dot);
        }
        vn += __shfl_xor(vn, 1); vn += __shfl_xor(vn, 2); vn += __shfl_xor(vn, 4);
        dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); dot += __shfl_xor(dot, 4);
        const float sq = sqrtf(vn / (float)V + 1e-5f), den = sq + 1e-5f;
        const float k2 = dot / (den * den) / ((float)V * sq);
        if (live)
            for (int u = sub; u < V; u += 8) {
                const float n2 = y[3 * u] * y[3 * u] + y[3 * u + 1] * y[3 * u + 1] + y[3 * u + 2] * y[3 * u + 2];
                const float lv = n2 > 1e-8f ? 1.0f : 0.f;
                const float m = wt_drop(p.c, (uint32_t)p.stream, n, S + u) * mul;
                for (int c = 0; c < 3; ++c) {
                    const float dy = eA[3 * u + c] + (eB ? eB[3 * u + c] : 0.f);
                    const float dx = dy / den - k2 * lv * y[3 * u + c];
                    p.out1_v[(size_t)n * V3 + 3 * u + c] = dx;
                    p.out2_v[(size_t)n * V3 + 3 * u + c] = dx * m;
                }
            }
        if constexpr (WG) {
            __syncthreads();
            if (sub == 0) { s_mean[r] = mean; s_rstd[r] = rstd; s_node[r] = n; }
            __syncthreads();
            // the norm's weight and bias: sums over the tile's rows in row order
            for (int f = tid; f < S; f += 256) {
                float sw = 0.f, sb = 0.f;
                for (int rr = 0; rr < tn; ++rr) {
                    const size_t o = (size_t)s_node[rr] * S + f;
                    const float dy = p.dyA_s[o] + (p.dyB_s ? p.dyB_s[o] : 0.f);
                    sw = fmaf(dy, (p.x_s[o] - s_mean[rr]) * s_rstd[rr], sw);
                    sb += dy;
                }
                gp[p.o_lw[nt] + f] += sw;
                gp[p.o_lb[nt] + f] += sb;
            }
            __syncthreads();
        }
    }
}

template <bool WG>
__global__ __launch_bounds__(256) void k_wt_head_out(const WtHeadOutParams p) {
    const int tid = threadIdx.x, nf = p.pharm_nf;
    const float* W = p.c.W;
    for (int i = blockIdx.x; i < p.Nf; i += gridDim.x) {
        const size_t n = (size_t)p.Np + i;
        if (tid < 64) {
            float acc = 0.f;
            for (int k = 0; k < nf; ++k) acc = fmaf(p.g_eps_h[(size_t)i * nf + k], W[p.o_Wout + k * 64 + tid], acc);
            p.up_s[n * p.up_ls + tid] = acc;
        } else if (tid < 67) p.up_v[n * p.up_lv + (tid - 64)] = p.g_eps_x[(size_t)i * 3 + (tid - 64)];
    }
    if constexpr (WG) {
        float* gp = p.c.gpart + (size_t)blockIdx.x * p.c.gstride;
        for (int idx = tid; idx < nf * 64; idx += 256) {
            const int k = idx >> 6, f = idx & 63;
            float acc = 0.f;
            for (int i = blockIdx.x; i < p.Nf; i += gridDim.x) acc = fmaf(p.g_eps_h[(size_t)i * nf + k], p.h64[(size_t)i * 64 + f], acc);
            gp[p.o_Wout + idx] += acc;
        }
        if (tid < nf) {
            float acc = 0.f;
            for (int i = blockIdx.x; i < p.Nf; i += gridDim.x) acc += p.g_eps_h[(size_t)i * nf + tid];
            gp[p.o_bout + tid] += acc;
        }
    }
}

// Linear(nf + 1 -> S) + SiLU + LayerNorm of every node (dynamics_gvp.py:107-117, 143-151): tiles of 32 nodes of one type,
// eight lanes per row; LDS: z (later the normalised rows) and dz [32][S + 1] each, the inputs [32][17]
// (WG false: only dL/d(the centers' feature rows) is wanted -- the protein tiles have nothing to do)
template <bool WG>
__global__ __launch_bounds__(256) void k_wt_encode(const WtEncParams p) {
    extern __shared__ float lds[];
    const int S = p.c.S, lz = S + 1, tid = threadIdx.x;
    float* zb = lds;
    float* dzb = zb + PFW_ROWS * lz;
    float* xin = dzb + PFW_ROWS * lz;
    float* gp = nullptr;
    if constexpr (WG) gp = p.c.gpart + (size_t)blockIdx.x * p.c.gstride;
    const float* W = p.c.W;
    const int tp = (p.Np + PFW_ROWS - 1) / PFW_ROWS, tf = (p.Nf + PFW_ROWS - 1) / PFW_ROWS;
    for (int ti = (WG ? 0 : tp) + blockIdx.x; ti < tp + tf; ti += gridDim.x) {
        const int nt = ti >= tp ? 1 : 0;
        const int n0 = nt ? p.Np + (ti - tp) * PFW_ROWS : ti * PFW_ROWS;
        const int tn = min(PFW_ROWS, (nt ? p.Np + p.Nf : p.Np) - n0);
        const int nf = nt ? p.pharm_nf : p.rec_nf, K = nf + 1;
        __syncthreads();
        for (int i = tid; i < PFW_ROWS * K; i += 256) {
            const int r = i / K, k = i - r * K, n = n0 + min(r, tn - 1);
            float x;
            if (k < nf) x = nt ? p.pharm_h[(size_t)(n - p.Np) * nf + k] : p.prot_h0[(size_t)n * nf + k];
            else x = p.t[p.gid[n]];
            xin[r * 17 + k] = x;
        }
        __syncthreads();
        const int r = tid >> 3, sub = tid & 7;
        const bool live = r < tn;
        const int n = n0 + min(r, tn - 1);
        const float* w = W + p.o_w[nt];
        float sum = 0.f;
        for (int f = sub; f < S; f += 8) {
            float acc = W[p.o_b[nt] + f];
            for (int k = 0; k < K; ++k) acc = fmaf(xin[r * 17 + k], w[f * K + k], acc);
            zb[r * lz + f] = acc;
            sum += acc * t_sigmoid(acc);
        }
        sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
        const float mean = sum / (float)S;
        float var = 0.f;
        for (int f = sub; f < S; f += 8) { const float zz = zb[r * lz + f]; const float c = zz * t_sigmoid(zz) - mean; var = fmaf(c, c, var); }
        var += __shfl_xor(var, 1); var += __shfl_xor(var, 2); var += __shfl_xor(var, 4);
        const float rstd = 1.0f / sqrtf(var / (float)S + 1e-5f);
        const float* dy = p.G_h + (size_t)n * S;
        const float* lw = W + p.o_lw[nt];
        float m1 = 0.f, m2 = 0.f;
        for (int f = sub; f < S; f += 8) {
            const float zz = zb[r * lz + f];
            const float g = dy[f] * lw[f];
            m1 += g; m2 = fmaf(g, (zz * t_sigmoid(zz) - mean) * rstd, m2);
        }
        m1 += __shfl_xor(m1, 1); m1 += __shfl_xor(m1, 2); m1 += __shfl_xor(m1, 4);
        m2 += __shfl_xor(m2, 1); m2 += __shfl_xor(m2, 2); m2 += __shfl_xor(m2, 4);
        m1 /= (float)S; m2 /= (float)S;
        for (int f = sub; f < S; f += 8) {
            const float zz = zb[r * lz + f], s = t_sigmoid(zz);
            const float xh = (zz * s - mean) * rstd;
            const float ga = rstd * (dy[f] * lw[f] - m1 - xh * m2);
            dzb[r * lz + f] = live ? ga * s * (1.0f + zz * (1.0f - s)) : 0.f;
            zb[r * lz + f] = live ? xh : 0.f;
        }
        __syncthreads();
        if constexpr (WG) {
            for (int idx = tid; idx < S * K; idx += 256) {
                const int f = idx / K, k = idx - f * K;
                float s = 0.f;
                for (int rr = 0; rr < tn; ++rr) s = fmaf(dzb[rr * lz + f], xin[rr * 17 + k], s);
                gp[p.o_w[nt] + idx] += s;
            }
            for (int f = tid; f < S; f += 256) {
                float sb = 0.f, sw = 0.f, sl = 0.f;
                for (int rr = 0; rr < tn; ++rr) {
                    const float d = p.G_h[(size_t)(n0 + rr) * S + f];
                    sb += dzb[rr * lz + f]; sw = fmaf(d, zb[rr * lz + f], sw); sl += d;
                }
                gp[p.o_b[nt] + f] += sb;
                gp[p.o_lw[nt] + f] += sw;
                gp[p.o_lb[nt] + f] += sl;
            }
        }
        if (nt && p.g_pharm_h)                  // dL/dh_t = dz W over the feature columns
            for (int idx = tid; idx < tn * nf; idx += 256) {
                const int rr = idx / nf, k = idx - rr * nf;
                float s = 0.f;
                for (int f = 0; f < S; ++f) s = fmaf(dzb[rr * lz + f], w[f * K + k], s);
                p.g_pharm_h[(size_t)(n0 - p.Np + rr) * nf + k] = s;
            }
    }
}

// one wave per center (WtCenterSumParams): every lane takes every 64th slot of a range, fp64 partial sums, one fixed tree at the end
// (also the tuned family's, pf_train_set_input_grads: it reads nothing of the wide workspace but g_diff, which the caller names)
__global__ __launch_bounds__(256) void k_wt_center_sum(const WtCenterSumParams p) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= p.Nf) return;
    const int n = p.Np + i, g = p.gid[n];
    double a[3] = {0.0, 0.0, 0.0};
    for (int l = 0; l < p.L; ++l) {
        const float* gd = p.g_diff + (size_t)l * p.layer_stride * 3;
        for (int k = 0; k < 2; ++k) {           // destination of its ff, then its pf in-edges
            const int st = p.in_start[k * p.N + n], c = p.in_cnt[k * p.N + n];
            for (int e = st + lane; e < st + c; e += 64)
                for (int q = 0; q < 3; ++q) a[q] -= (double)gd[(size_t)e * 3 + q];
        }
        for (int k = 0; k < 2; ++k) {           // source among its graph's ff, then fp slots
            const int et = k == 0 ? ET_FF : ET_FP;
            const int st = p.reg[et * p.B + g], c = p.dyn_cnt[et * p.B + g];
            for (int e = st + lane; e < st + c; e += 64)
                if (p.esrc[e] == n)
                    for (int q = 0; q < 3; ++q) a[q] += (double)gd[(size_t)e * 3 + q];
        }
    }
    for (int q = 0; q < 3; ++q) {
        double s = a[q];
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) p.g_x[(size_t)i * 3 + q] = (float)s;
    }
}

__global__ __launch_bounds__(256) void k_wt_reduce(const float* gpart, const int gstride, const int nb, float* grad, const int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += gpart[(size_t)b * gstride + i];
    grad[i] = s;
}

}  // namespace

extern "C" {
size_t pfk_wt_chain_lds_bytes(int S, int V, int edge) { return wt_chain_lds_floats(S, V, edge != 0) * sizeof(float); }

// wgrad: 1 the full pass, 0 the inputs-only pass (no weight-gradient products: c.gpart is not read)
void pfk_wt_chain(const WtChainParams* p, int edge, int wgrad, hipStream_t s) {
    if (p->n_tiles == 0) return;
    const size_t bytes = pfk_wt_chain_lds_bytes(p->c.S, p->c.V, edge);
    const int grid = std::min(PFWT_NB, p->n_tiles);
    auto go = [&](auto kern) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), bytes, s, *p);
    };
    if (wgrad) { if (edge) go(k_wt_chain<true, true>); else go(k_wt_chain<false, true>); }
    else { if (edge) go(k_wt_chain<true, false>); else go(k_wt_chain<false, false>); }
}
void pfk_wt_norm(const WtNormParams* p, int wgrad, hipStream_t s) {
    if (p->n_tiles == 0) return;
    if (wgrad) hipLaunchKernelGGL(k_wt_norm<true>, dim3(std::min(PFWT_NB, p->n_tiles)), dim3(256), 0, s, *p);
    else hipLaunchKernelGGL(k_wt_norm<false>, dim3(std::min(PFWT_NB, p->n_tiles)), dim3(256), 0, s, *p);
}
void pfk_wt_head_out(const WtHeadOutParams* p, int wgrad, hipStream_t s) {
    if (p->Nf == 0) return;
    if (wgrad) hipLaunchKernelGGL(k_wt_head_out<true>, dim3(std::min(PFWT_NB, p->Nf)), dim3(256), 0, s, *p);
    else hipLaunchKernelGGL(k_wt_head_out<false>, dim3(std::min(PFWT_NB, p->Nf)), dim3(256), 0, s, *p);
}
void pfk_wt_encode(const WtEncParams* p, int wgrad, hipStream_t s) {
    const int tiles = (wgrad ? (p->Np + PFW_ROWS - 1) / PFW_ROWS : 0) + (p->Nf + PFW_ROWS - 1) / PFW_ROWS;
    if (tiles == 0) return;
    const size_t bytes = ((size_t)2 * PFW_ROWS * (p->c.S + 1) + PFW_ROWS * 17) * sizeof(float);
    auto go = [&](auto kern) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        hipLaunchKernelGGL(kern, dim3(std::min(PFWT_NB, tiles)), dim3(256), bytes, s, *p);
    };
    if (wgrad) go(k_wt_encode<true>); else go(k_wt_encode<false>);
}
void pfk_wt_center_sum(const WtCenterSumParams* p, hipStream_t s) {
    if (p->Nf == 0) return;
    hipLaunchKernelGGL(k_wt_center_sum, dim3((p->Nf + 3) / 4), dim3(256), 0, s, *p);
}
void pfk_wt_reduce(const float* gpart, int gstride, float* grad, int nparams, hipStream_t s) {
    if (nparams == 0) return;
    hipLaunchKernelGGL(k_wt_reduce, dim3((nparams + 255) / 256), dim3(256), 0, s, gpart, gstride, PFWT_NB, grad, nparams);
}
}
