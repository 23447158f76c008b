// The pocket field of a guided step (pf_guide_field_next): clash and complementarity energies on the predicted
// clean centers and their gradients, added into what k_guide_grad left.
//   x0_hat = (x_t - sigma_t eps_x) / alpha_t (noise parameterisation) or eps_x (endpoint);  y_f = x0_hat[f] + D[g]
//   clash, sampler's frame (x0_hat against the current protein rows a_i):  E += w_clash max(0, r_i - rho)^2,  rho = |x0_hat - a_i|
//   complementarity, caller's frame (y against the receptor features q_j), per type t with a non-empty S_t = {j : match[t][u_j]}:
//     rho~ = rho_min - log(sum_j exp(-kappa (rho_j - rho_min))) / kappa,  m = max(0, rho~ - dist[t]),  E += w_comp p_ft m^2
//     p_f = softmax_t(type_sharpness * h0_hat[f]),  h0_hat = (h_t - sigma_t eps_h) / alpha_t or eps_h: a constant of the gradient
// One workgroup of 256 threads per graph.  Wave w owns the centers f0 + w, f0 + w + 4, ...; for one center its 64 lanes walk the
// graph's atoms, then the graph's features, i ascending in steps of 64.  Every sum has one order: a lane's terms in ascending i,
// the 64 lanes by the xor butterfly (offsets 32 .. 1), a wave's centers in ascending f, the four waves as (w0 + w1) + (w2 + w3) in
// LDS.  No atomics: the same bits on every run.  Squared distances and every product that feeds a sum are formed with FP
// contraction off (as in pf_restraint).
// A launch starts with cold caches: after the graph's pointers, a lane's first 8 atom rows and radii (512 atoms stay in registers
// for all of the wave's centers), the wave's first center rows, its first feature and D are all requested before the first wait
// (4.12.1 of DESIGN.md).
#include <hip/hip_runtime.h>
#include "pf_device.h"
#include "pf_field.h"

#define FIELD_NA 8      // atom rows a lane keeps in registers

__device__ __forceinline__ float field_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float field_wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float field_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// x0_hat and y of one center (pf_guide_y's operations)
__device__ __forceinline__ void field_x0(const float x[3], const float e[3], const float D[3], const float alpha_t, const float sigma_t,
                                         const int ep_coord, float x0[3], float y[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (ep_coord) x0[c] = e[c];
        else { const float se = sigma_t * e[c], d = x[c] - se; x0[c] = d / alpha_t; }
        y[c] = x0[c] + D[c];
    }
}
// one (center, atom) pair: returns its energy and adds dE/dx0 into g.  r == 0 (an inert atom, or a lane without one): exact zeros
__device__ __forceinline__ float field_clash(const float x0[3], const float4 a, const float r, const float w, float g[3]) {
#pragma clang fp contract(off)
    const float dx = x0[0] - a.x, dy = x0[1] - a.y, dz = x0[2] - a.z;
    const float rho = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float m = fmaxf(0.f, r - rho);
    if (rho > 0.f && m > 0.f) {
        const float c = ((2.0f * w) * m) / rho;
        const float gx = c * dx, gy = c * dy, gz = c * dz;
        g[0] -= gx; g[1] -= gy; g[2] -= gz;
    }
    return w * (m * m);
}
__device__ __forceinline__ float field_rho(const float y[3], const float4 ft, float d[3]) {
#pragma clang fp contract(off)
    d[0] = y[0] - ft.x; d[1] = y[1] - ft.y; d[2] = y[2] - ft.z;
    return sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// TYPES (pf_guide_types_next with comp_types): the complementarity energy also leaves its gradient w.r.t. the predicted clean
// features, dE/dh0_hat[f][k] = w_comp s p_fk (m_k^2 - sum_t p_ft m_t^2), from the m_t and p_ft the loop holds anyway -- lane t owns
// type t.  A type whose set is empty in the graph takes m_t = unmatched there, and its energy goes to E_type, not to E3.  The
// false form is the code as it was
template <bool TYPES>
__device__ __forceinline__ void guide_field_body(const StepParams& p, const FieldParams& q, const FieldTypeParams* ft) {
    __shared__ float s_e[4][3];
    __shared__ int s_row[PF_FIELD_MAX_TYPES];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = p.nf;
    const int f0 = p.pharm_ptr[g], f1 = p.pharm_ptr[g + 1];
    const int p0 = p.prot_ptr[g], p1 = p.prot_ptr[g + 1];
    const int j0 = q.ph_ptr[g], j1 = q.ph_ptr[g + 1];
    // ---- every first row, before the first wait ----
    float4 at[FIELD_NA]; float ar[FIELD_NA];
#pragma unroll
    for (int k = 0; k < FIELD_NA; ++k) {
        const int i = p0 + lane + 64 * k;
        const bool ok = i < p1;
        at[k] = ok ? p.xn[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        ar[k] = ok ? q.atom_r[i] : 0.f;
    }
    const int fa = f0 + wave;
    const bool own = fa < f1;
    float4 xa = make_float4(0.f, 0.f, 0.f, 0.f);
    float ea[3] = {0.f, 0.f, 0.f}, hva = 0.f, eha = 0.f;
    if (own) {
        xa = p.xn[p.Np_tot + fa];
        for (int c = 0; c < 3; ++c) ea[c] = p.eps_x[(size_t)fa * 3 + c];
        if (lane < nt) { hva = p.pharm_h[(size_t)fa * nt + lane]; eha = p.eps_h[(size_t)fa * nt + lane]; }
    }
    float4 qa = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j0 + lane < j1) qa = q.ph_xt[j0 + lane];
    const float D[3] = {q.D[3 * g], q.D[3 * g + 1], q.D[3 * g + 2]};
    if (tid < nt) {                                     // row t of the match table as a bit mask over the receptor types
        int bits = 0;
        for (int u = 0; u < nt; ++u) bits |= (q.match[tid * nt + u] != 0) << u;
        s_row[tid] = bits;
    }
    {
        float touch = ((xa.x + xa.y) + (xa.z + ea[0])) + ((ea[1] + ea[2]) + (hva + eha)) + (qa.x + D[0]);
#pragma unroll
        for (int k = 0; k < FIELD_NA; ++k) touch += at[k].x + ar[k];
        asm volatile("" :: "v"(touch) : "memory");
    }
    __syncthreads();
    float e_clash = 0.f, e_comp = 0.f, e_un = 0.f;      // this wave's centers, f ascending
    for (int f = fa; f < f1; f += 4) {
        float x[3] = {xa.x, xa.y, xa.z}, e[3] = {ea[0], ea[1], ea[2]}, hv = hva, eh = eha;
        if (f != fa) {
            const float4 xv = p.xn[p.Np_tot + f];
            x[0] = xv.x; x[1] = xv.y; x[2] = xv.z;
            for (int c = 0; c < 3; ++c) e[c] = p.eps_x[(size_t)f * 3 + c];
            hv = 0.f; eh = 0.f;
            if (lane < nt) { hv = p.pharm_h[(size_t)f * nt + lane]; eh = p.eps_h[(size_t)f * nt + lane]; }
        }
        float x0[3], y[3];
        field_x0(x, e, D, q.alpha_t, q.sigma_t, q.ep_coord, x0, y);
        // ---- clash: this center against every atom of the graph ----
        float ec = 0.f, gc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < FIELD_NA; ++k) ec += field_clash(x0, at[k], ar[k], q.w_clash, gc);
        for (int i = p0 + lane + 64 * FIELD_NA; i < p1; i += 64) ec += field_clash(x0, p.xn[i], q.atom_r[i], q.w_clash, gc);
        ec = field_wave_sum(ec);
        gc[0] = field_wave_sum(gc[0]); gc[1] = field_wave_sum(gc[1]); gc[2] = field_wave_sum(gc[2]);
        // ---- complementarity: per type t, the soft minimum over the matching features ----
        float em = 0.f, gm[3] = {0.f, 0.f, 0.f};
        float eu = 0.f, m2 = 0.f;                       // TYPES: the unmatched energy; lane t: m_t^2
        if (TYPES || j1 > j0) {
            float pl;                                   // lane t < nt: p_ft
            {
#pragma clang fp contract(off)
                float h0 = eh;
                if (!q.ep_feat) { const float se = q.sigma_t * eh, d = hv - se; h0 = d / q.alpha_t; }
                const float v = lane < nt ? q.type_sharpness * h0 : -INFINITY;
                const float mx = field_wave_max(v);
                const float ex = lane < nt ? expf(v - mx) : 0.f;
                pl = ex / field_wave_sum(ex);
            }
            for (int t = 0; t < nt; ++t) {
#pragma clang fp contract(off)
                const int row = s_row[t];
                const float pt = __shfl(pl, t);
                float mn = INFINITY;
                for (int j = j0 + lane; j < j1; j += 64) {
                    const float4 ft = j == j0 + lane ? qa : q.ph_xt[j];
                    if (!((row >> __float_as_int(ft.w)) & 1)) continue;
                    float d[3];
                    mn = fminf(mn, field_rho(y, ft, d));
                }
                mn = field_wave_min(mn);
                if (mn == INFINITY) {                   // S_t is empty in this graph (the same value in every lane)
                    if constexpr (TYPES) {
                        const float u2 = ft->unmatched * ft->unmatched;
                        const float wp = q.w_comp * pt;
                        const float et = wp * u2;
                        eu += et;
                        if (lane == t) m2 = u2;
                    }
                    continue;
                }
                float Z = 0.f, V[3] = {0.f, 0.f, 0.f};
                for (int j = j0 + lane; j < j1; j += 64) {
                    const float4 ft = j == j0 + lane ? qa : q.ph_xt[j];
                    if (!((row >> __float_as_int(ft.w)) & 1)) continue;
                    float d[3];
                    const float rho = field_rho(y, ft, d);
                    const float a = q.kappa * (rho - mn);
                    const float wj = expf(-a);
                    Z += wj;
                    if (rho > 0.f) {
                        const float c = wj / rho;
                        const float vx = c * d[0], vy = c * d[1], vz = c * d[2];
                        V[0] += vx; V[1] += vy; V[2] += vz;
                    }
                }
                Z = field_wave_sum(Z);
                V[0] = field_wave_sum(V[0]); V[1] = field_wave_sum(V[1]); V[2] = field_wave_sum(V[2]);
                const float soft = mn - logf(Z) / q.kappa;
                const float m = fmaxf(0.f, soft - q.dist[t]);
                const float wp = q.w_comp * pt;
                const float et = wp * (m * m);
                em += et;
                if constexpr (TYPES) { if (lane == t) m2 = m * m; }
                const float c = (wp * (2.0f * m)) / Z;
                const float ax = c * V[0], ay = c * V[1], az = c * V[2];
                gm[0] += ax; gm[1] += ay; gm[2] += az;
            }
            if constexpr (TYPES) {
#pragma clang fp contract(off)
                const float pm = lane < nt ? pl * m2 : 0.f;
                const float mean = field_wave_sum(pm);
                if (lane < nt) {
                    const float ws = q.w_comp * q.type_sharpness;
                    const float gh = (ws * pl) * (m2 - mean);
                    // (phi_h / phi_x): the factor the VJP's g_eps_h carries, see pf_denoise_step_guided
                    const float ratio = q.sigma_t / q.alpha_t;
                    const float ph = q.ep_feat ? 1.0f : -ratio, px = q.ep_coord ? 1.0f : -ratio;
                    ft->g0_h[(size_t)f * nt + lane] = gh;
                    ft->gs_h[(size_t)f * nt + lane] = (ph / px) * gh;
                }
            }
        }
        if (lane == 0) {
#pragma clang fp contract(off)
            for (int c = 0; c < 3; ++c) {
                const float r = q.g0[(size_t)f * 3 + c];
                q.g0[(size_t)f * 3 + c] = (r + gc[c]) + gm[c];
            }
            e_clash += ec; e_comp += em;
            if constexpr (TYPES) e_un += eu;
        }
    }
    if (lane == 0) { s_e[wave][0] = e_clash; s_e[wave][1] = e_comp; if constexpr (TYPES) s_e[wave][2] = e_un; }
    __syncthreads();
    if (tid == 0) {
        const float er = q.energy[g];
        const float ec = (s_e[0][0] + s_e[1][0]) + (s_e[2][0] + s_e[3][0]);
        const float em = (s_e[0][1] + s_e[1][1]) + (s_e[2][1] + s_e[3][1]);
        float tot = (er + ec) + em;
        if constexpr (TYPES) {
            const float et = (s_e[0][2] + s_e[1][2]) + (s_e[2][2] + s_e[3][2]);
            ft->E_type[g] = et;
            tot = tot + et;
        }
        q.E3[3 * g] = er; q.E3[3 * g + 1] = ec; q.E3[3 * g + 2] = em;
        q.energy[g] = tot;
        if (q.traj_energy) q.traj_energy[g] = tot;
    }
}

__global__ __launch_bounds__(256) void k_guide_field(const StepParams p, const FieldParams q) { guide_field_body<false>(p, q, nullptr); }
__global__ __launch_bounds__(256) void k_guide_field_types(const StepParams p, const FieldParams q, const FieldTypeParams ft) {
    guide_field_body<true>(p, q, &ft);
}

// ---------------------------------------------------------------------------------------------
// Type restraints (pf_guide_types_next), behind k_guide_grad and k_guide_field:
//   h0_hat = (h_t - sigma_t eps_h) / alpha_t or eps_h;  v_k = s h0_hat[k];  p_f = softmax(v)  (the maximum subtracted first)
//   restraint (center, c, pt, r, w):  omega = 1 (r == 0) or q^2, q = max(0, 1 - rho^2 / r^2), rho^2 = |y_f - pt|^2
//     CE = log(sum_k exp(v_k - max)) + max - v_c;  E = w omega CE;  dE/dh0_hat[k] = (w omega s)(p_fk - [k == c])
//     dE/dy_f = (w CE)(2 q)(-2 (y_f - pt) / r^2): exact zeros when r == 0 or q == 0
// One workgroup of 256 threads per graph.  Wave w owns the centers f0 + w, f0 + w + 4, ...; lane k < nf is type k; every lane
// walks the graph's restraints in ascending j (the window and CE are the same value in every lane).  Lane 0 adds the windows'
// coordinate term into g0[f] behind what k_guide_grad and k_guide_field left; lane k stores g0_h[f][k] -- the restraints' term,
// then the complementarity term the TYPES form of k_guide_field left there (q.E3 set) -- and gs_h = (phi_h / phi_x) g0_h.  A
// wave's energy: its centers in ascending f, j ascending; the four waves as (w0 + w1) + (w2 + w3) in LDS; thread 0 rewrites E[g]
// and the trajectory row as (((E_restr + E_clash) + E_comp) + E_type).  No atomics.  One rounding per operation.
// A launch starts with cold caches: after the graph's pointers the wave's first center rows, D and the first restraint are all
// requested before the first wait (4.12.1 of DESIGN.md).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_guide_types(const StepParams p, const TypeParams q) {
    __shared__ float s_e[4];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = p.nf;
    const int f0 = p.pharm_ptr[g], f1 = p.pharm_ptr[g + 1];
    const int r0 = q.ptr[g], r1 = q.ptr[g + 1];
    const int fa = f0 + wave;
    const bool own = fa < f1, typ = lane < nt;
    float4 xa = make_float4(0.f, 0.f, 0.f, 0.f);
    float ea[3] = {0.f, 0.f, 0.f}, hva = 0.f, eha = 0.f;
    if (own) {
        xa = p.xn[p.Np_tot + fa];
        for (int c = 0; c < 3; ++c) ea[c] = p.eps_x[(size_t)fa * 3 + c];
        if (typ) { hva = p.pharm_h[(size_t)fa * nt + lane]; eha = p.eps_h[(size_t)fa * nt + lane]; }
    }
    const float D[3] = {q.D[3 * g], q.D[3 * g + 1], q.D[3 * g + 2]};
    int c0 = 0; float w0 = 0.f;
    if (r1 > r0) { c0 = q.center[r0]; w0 = q.w[r0]; }
    asm volatile("" :: "v"(((xa.x + xa.y) + (xa.z + ea[0])) + ((ea[1] + ea[2]) + (hva + eha)) + (D[0] + w0)), "v"(c0) : "memory");
    float e_wave = 0.f;
    for (int f = fa; f < f1; f += 4) {
#pragma clang fp contract(off)
        float x[3] = {xa.x, xa.y, xa.z}, e[3] = {ea[0], ea[1], ea[2]}, hv = hva, eh = eha;
        if (f != fa) {
            const float4 xv = p.xn[p.Np_tot + f];
            x[0] = xv.x; x[1] = xv.y; x[2] = xv.z;
            for (int c = 0; c < 3; ++c) e[c] = p.eps_x[(size_t)f * 3 + c];
            hv = 0.f; eh = 0.f;
            if (typ) { hv = p.pharm_h[(size_t)f * nt + lane]; eh = p.eps_h[(size_t)f * nt + lane]; }
        }
        float x0[3], y[3];
        field_x0(x, e, D, q.alpha_t, q.sigma_t, q.ep_coord, x0, y);
        float h0 = eh;
        if (!q.ep_feat) { const float se = q.sigma_t * eh, d = hv - se; h0 = d / q.alpha_t; }
        const float v = typ ? q.sharp * h0 : -INFINITY;
        const float mx = field_wave_max(v);
        const float ex = typ ? expf(v - mx) : 0.f;
        const float Z = field_wave_sum(ex);
        const float pl = ex / Z;
        const float lse = logf(Z) + mx;
        float gh = 0.f, gy[3] = {0.f, 0.f, 0.f}, ef = 0.f;
        for (int j = r0; j < r1; ++j) {
            const int ci = q.center[j];
            if (ci >= 0 && ci != f - f0) continue;
            const int ct = q.type[j];
            const float r = q.r[j], w = q.w[j];
            const float CE = lse - __shfl(v, ct);
            float omega = 1.0f;
            if (r > 0.f) {
                const float dx = y[0] - q.p[(size_t)j * 3], dy = y[1] - q.p[(size_t)j * 3 + 1], dz = y[2] - q.p[(size_t)j * 3 + 2];
                const float rho2 = (dx * dx + dy * dy) + dz * dz;
                const float r2 = r * r;
                const float qq = fmaxf(0.f, 1.0f - rho2 / r2);
                omega = qq * qq;
                if (qq > 0.f) {
                    const float k = (w * CE) * (2.0f * qq);
                    const float ax = k * ((-2.0f * dx) / r2), ay = k * ((-2.0f * dy) / r2), az = k * ((-2.0f * dz) / r2);
                    gy[0] += ax; gy[1] += ay; gy[2] += az;
                }
            }
            const float wo = w * omega;
            const float ej = wo * CE;
            ef += ej;
            const float t = (wo * q.sharp) * (pl - (lane == ct ? 1.0f : 0.f));
            gh += t;
        }
        e_wave += ef;
        if (lane == 0) {
            for (int c = 0; c < 3; ++c) {
                const float b = q.g0[(size_t)f * 3 + c];
                q.g0[(size_t)f * 3 + c] = b + gy[c];
            }
        }
        if (typ) {
            if (q.E3) gh = gh + q.g0_h[(size_t)f * nt + lane];
            const float ratio = q.sigma_t / q.alpha_t;
            const float ph = q.ep_feat ? 1.0f : -ratio, px = q.ep_coord ? 1.0f : -ratio;
            q.g0_h[(size_t)f * nt + lane] = gh;
            q.gs_h[(size_t)f * nt + lane] = (ph / px) * gh;
        }
    }
    if (lane == 0) s_e[wave] = e_wave;
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        float et = (s_e[0] + s_e[1]) + (s_e[2] + s_e[3]);
        float base = q.energy[g];
        if (q.E3) {
            et = et + q.E_type[g];
            base = (q.E3[3 * g] + q.E3[3 * g + 1]) + q.E3[3 * g + 2];
        }
        const float tot = base + et;
        q.E_type[g] = et;
        q.energy[g] = tot;
        if (q.traj_energy) q.traj_energy[g] = tot;
    }
}

extern "C" void pfk_guide_field(const StepParams* p, const FieldParams* q, hipStream_t s) {
    if (p->B <= 0) return;
    hipLaunchKernelGGL(k_guide_field, dim3(p->B), dim3(256), 0, s, *p, *q);
}
extern "C" void pfk_guide_field_types(const StepParams* p, const FieldParams* q, const FieldTypeParams* ft, hipStream_t s) {
    if (p->B <= 0) return;
    hipLaunchKernelGGL(k_guide_field_types, dim3(p->B), dim3(256), 0, s, *p, *q, *ft);
}
extern "C" void pfk_guide_types(const StepParams* p, const TypeParams* q, hipStream_t s) {
    if (p->B <= 0) return;
    hipLaunchKernelGGL(k_guide_types, dim3(p->B), dim3(256), 0, s, *p, *q);
}
