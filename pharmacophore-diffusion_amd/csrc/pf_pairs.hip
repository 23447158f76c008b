// Pair guidance of a guided step (pf_guide_pairs_next): distance restraints between two centers of one graph on the
// predicted clean centers, behind k_guide_grad, k_guide_field and k_guide_types.
//   y_f = x0_hat[f] + D[g] (pf_guide_y's operations) for a free center, pin_x[f] for a position-pinned one (flag bit 0)
//   restraint (i, j, lo, hi, w), -1: every center.  A covered pair {a, b}: d = y_a - y_b, rho = |d|,
//     m_lo = max(0, lo - rho), m_hi = max(0, rho - hi) (hi = +inf: 0),  E = w (m_lo^2 + m_hi^2)
//     dE/dy_a = ((2 w)(m_hi - m_lo) / rho) d = -dE/dy_b;  rho == 0: no gradient
// One workgroup of 256 threads per graph; a graph has at most 64 centers.  Wave 0 stages the graph's y rows and pin bits in LDS once.
// Then thread (wave s, lane c) is center c's quarter s: it walks the graph's restraints in ascending order and, within a
// restraint, center c's covered partners b with (b & 3) == s in ascending order, adding every dE/dy_c into one accumulator and
// every E with c < b into another.  The four quarters meet in LDS as (s0 + s1) + (s2 + s3): that is g_pair[c] (exact zeros for a
// position-pinned center) and e_c.  Thread 0 sums E_pair = sum_c e_c, c ascending, and rewrites E[g] and the trajectory row as
// (E so far) + E_pair.  No atomics, plain vector stores: the same bits on every run.  One rounding per operation (FP contraction
// off, as in pf_restraint).
// A launch starts with cold caches: after the graph's pointers the center's rows, its pin row, D and the first restraint are all
// requested before the first wait (4.12.1 of DESIGN.md).
#include <hip/hip_runtime.h>
#include "pf_device.h"
#include "pf_pairs.h"

__global__ __launch_bounds__(256) void k_guide_pairs(const StepParams p, const PairParams q) {
    __shared__ float s_y[PF_PAIRS_MAX_CENTERS][3];
    __shared__ int s_pin[PF_PAIRS_MAX_CENTERS];
    __shared__ float s_part[4][PF_PAIRS_MAX_CENTERS][4];        // per quarter and center: dE/dy [3], e
    __shared__ float s_e[PF_PAIRS_MAX_CENTERS];
    const int g = blockIdx.x, tid = threadIdx.x, c = tid & 63, s = tid >> 6;
    const int f0 = p.pharm_ptr[g], f1 = p.pharm_ptr[g + 1];
    const int r0 = q.ptr[g], r1 = q.ptr[g + 1];
    const int n = min(f1 - f0, PF_PAIRS_MAX_CENTERS);
    const int f = f0 + c;
    const bool own = c < n, stage = own && s == 0;
    float4 xa = make_float4(0.f, 0.f, 0.f, 0.f);
    float ea[3] = {0.f, 0.f, 0.f}, px[3] = {0.f, 0.f, 0.f};
    int flag = 0;
    if (stage) {
        xa = p.xn[p.Np_tot + f];
        flag = q.flags[f];
        for (int k = 0; k < 3; ++k) { ea[k] = p.eps_x[(size_t)f * 3 + k]; px[k] = q.pin_x[(size_t)f * 3 + k]; }
    }
    const float D[3] = {q.D[3 * g], q.D[3 * g + 1], q.D[3 * g + 2]};
    int i0 = 0; float w0 = 0.f;
    if (r1 > r0) { i0 = q.i[r0]; w0 = q.w[r0]; }
    asm volatile("" :: "v"(((xa.x + xa.y) + (xa.z + ea[0])) + ((ea[1] + ea[2]) + (px[0] + px[1])) + ((px[2] + D[0]) + w0)), "v"(flag + i0) : "memory");
    if (stage) {
#pragma clang fp contract(off)
        const float x[3] = {xa.x, xa.y, xa.z};
        for (int k = 0; k < 3; ++k) {
            float x0;
            if (q.ep_coord) x0 = ea[k];
            else { const float se = q.sigma_t * ea[k], d = x[k] - se; x0 = d / q.alpha_t; }
            const float y = x0 + D[k];
            s_y[c][k] = (flag & 1) ? px[k] : y;
        }
        s_pin[c] = flag & 1;
    }
    __syncthreads();
    float acc[3] = {0.f, 0.f, 0.f}, e = 0.f;
    if (own) {
#pragma clang fp contract(off)
        const float y[3] = {s_y[c][0], s_y[c][1], s_y[c][2]};
        for (int k = r0; k < r1; ++k) {
            const int ri = q.i[k], rj = q.j[k];
            const float lo = q.lo[k], hi = q.hi[k], w = q.w[k];
            int b0 = 0, b1 = n;                         // both wildcards: every other center
            if (ri >= 0 && rj >= 0) {                   // the pair {ri, rj}
                b0 = c == ri ? rj : c == rj ? ri : 0;
                b1 = c == ri || c == rj ? b0 + 1 : 0;
            } else if (ri >= 0 || rj >= 0) {            // {c0, b} for every b
                const int c0 = ri >= 0 ? ri : rj;
                if (c != c0) { b0 = c0; b1 = c0 + 1; }
            }
            b1 = min(b1, n);
            for (int b = b0 + ((s - b0) & 3); b < b1; b += 4) {
                if (b == c) continue;
                const float dx = y[0] - s_y[b][0], dy = y[1] - s_y[b][1], dz = y[2] - s_y[b][2];
                const float rho = sqrtf((dx * dx + dy * dy) + dz * dz);
                const float m_lo = fmaxf(0.f, lo - rho), m_hi = fmaxf(0.f, rho - hi);
                if (rho > 0.f) {
                    const float cf = ((2.0f * w) * (m_hi - m_lo)) / rho;
                    const float gx = cf * dx, gy = cf * dy, gz = cf * dz;
                    acc[0] += gx; acc[1] += gy; acc[2] += gz;
                }
                if (c < b) {
                    const float eb = w * (m_lo * m_lo + m_hi * m_hi);
                    e += eb;
                }
            }
        }
        s_part[s][c][0] = acc[0]; s_part[s][c][1] = acc[1]; s_part[s][c][2] = acc[2]; s_part[s][c][3] = e;
    }
    __syncthreads();
    if (stage) {
#pragma clang fp contract(off)
        const bool pinned = s_pin[c] != 0;
        for (int k = 0; k < 3; ++k) {
            const float t = (s_part[0][c][k] + s_part[1][c][k]) + (s_part[2][c][k] + s_part[3][c][k]);
            const float gp = pinned ? 0.f : t;
            const float b = q.g0[(size_t)f * 3 + k];
            q.g_pair[(size_t)f * 3 + k] = gp;
            q.g0[(size_t)f * 3 + k] = b + gp;
        }
        s_e[c] = (s_part[0][c][3] + s_part[1][c][3]) + (s_part[2][c][3] + s_part[3][c][3]);
    }
    for (int fz = f0 + PF_PAIRS_MAX_CENTERS + tid; fz < f1; fz += 256)         // (never bound: a graph has at most 64 centers)
        for (int k = 0; k < 3; ++k) q.g_pair[(size_t)fz * 3 + k] = 0.f;
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        float E = 0.f;
        for (int k = 0; k < n; ++k) E += s_e[k];
        const float tot = q.energy[g] + E;
        q.E_pair[g] = E;
        q.energy[g] = tot;
        if (q.traj_energy) q.traj_energy[g] = tot;
    }
}

extern "C" void pfk_guide_pairs(const StepParams* p, const PairParams* q, hipStream_t s) {
    if (p->B <= 0) return;
    hipLaunchKernelGGL(k_guide_pairs, dim3(p->B), dim3(256), 0, s, *p, *q);
}
