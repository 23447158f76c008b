// pf_stepmove.h -- the move a sampler step ends with, on the device: ONE skeleton (step_move_body) for every run kind, one graph per
// workgroup of 256 threads.  A move -- plain, multistep, pinned, guided, guided with types, re-noise, seed -- is a small struct below:
// what it reads, its arithmetic per value, its side outputs.  The skeleton owns everything the moves share:
//   * center f0 + lane of graph g belongs to lane `lane` of wave 0 (the bind rejects a graph of more than PF_MAXF centers);
//   * a launch starts with cold caches and a dependent global round trip is its unit of cost: after the graph's four
//     pointers every row the thread needs is requested before the first wait, and the new coordinates stay in registers across the
//     barriers of the COM reduction;
//   * frame_offset: D[g] of the moves that read values in the caller's frame; com_remove: the COM of the new centers and its removal.
// Both reductions are written once, in the orders every form of a step shares (the runs are bitwise repeatable across forms).
#pragma once
#include "pf_device.h"

static_assert(PF_MAXF <= 64, "the centers of a graph are the first lanes of wave 0");

// a value noised to a level, a * v + s * noise: a pinned center or a seed at this step's level, the re-noise move.  One rounding per
// operation, as in pf_feat_update
__device__ __forceinline__ float pf_noised_value(const float v, const float nz, const float a, const float s) {
#pragma clang fp contract(off)
    const float av = a * v, n = s * nz;
    return av + n;
}
// The guided step's move (reconstruction guidance, pf_denoise_step_guided) for one center: the gradient of the restraint energy
// w.r.t. x_t from g0 = dE/dy and the dynamics' VJP J(g0), the shift of the posterior mean, and its clip.  One rounding per
// operation, like pf_feat_update.  gr / sh: what the step applies (also stored for pf_debug_last_guidance)
__device__ __forceinline__ void pf_guide_shift(const float* g0, const float* jx, const float alpha_t, const float sigma_t, const int ep_coord,
                                               const float sigma_post, const float scale, const float clip, float* gr, float* sh) {
#pragma clang fp contract(off)
    const float ratio = sigma_t / alpha_t;
    const float s2 = sigma_post * sigma_post;
    const float k = scale * s2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (ep_coord) gr[c] = jx[c];
        else { const float a = g0[c] / alpha_t, b = ratio * jx[c]; gr[c] = a - b; }
        sh[c] = k * gr[c];
    }
    const float n = sqrtf((sh[0] * sh[0] + sh[1] * sh[1]) + sh[2] * sh[2]);
    if (clip > 0.f && n > clip) {
        const float f = clip / n;
        sh[0] *= f; sh[1] *= f; sh[2] *= f;
    }
}
// The feature half of the guided move (type guidance, pf_guide_types_next) for one center's row of nf entries:
//   grad_h = [g0_h / alpha_t, noise parameterisation of the features only] + phi_x J_h,  phi_x = -sigma_t / alpha_t or 1 (endpoint coordinates)
//   shift_h = (feat_scale sigma_post^2) grad_h, clipped to the Euclidean norm `clip` over the row
// It stores grad_h and the UNCLIPPED shift_h and returns the clip's factor (1: no clip).  One rounding per operation; the norm sums k ascending
__device__ __forceinline__ float pf_guide_shift_h(const float* g0h, const float* jh, const int nf, const float alpha_t, const float sigma_t,
                                                  const int ep_coord, const int ep_feat, const float sigma_post, const float scale,
                                                  const float clip, float* gr, float* sh) {
#pragma clang fp contract(off)
    const float ratio = sigma_t / alpha_t;
    const float s2 = sigma_post * sigma_post;
    const float k = scale * s2;
    float n2 = 0.f;
    for (int c = 0; c < nf; ++c) {
        const float j = jh[c];
        float b;
        if (ep_coord) b = j;
        else { const float rj = ratio * j; b = -rj; }
        float gv = b;
        if (!ep_feat) { const float a = g0h[c] / alpha_t; gv = a + b; }
        const float sv = k * gv;
        gr[c] = gv; sh[c] = sv;
        const float q = sv * sv;
        n2 += q;
    }
    const float n = sqrtf(n2);
    return (clip > 0.f && n > clip) ? clip / n : 1.0f;
}

// D[g] = c_init - mean of the graph's CURRENT protein rows (pf_sample_frame's rule): what takes a value of the caller's frame into the
// sampler's.  Wave 0 calls it; the sum is k_segment_mean's -- lane's rows at stride 64, the xor butterfly -- so every lane returns the
// same bits.  pa: row p0 + lane, requested by the caller before its first wait
__device__ __forceinline__ void frame_offset(const float4* xn, const int p0, const int p1, const int lane, const float4 pa, const float ci[3],
                                             float d[3]) {
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (p0 + lane < p1) { ax += pa.x; ay += pa.y; az += pa.z; }
    for (int i = p0 + lane + 64; i < p1; i += 64) { const float4 x = xn[i]; ax += x.x; ay += x.y; az += x.z; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); az += __shfl_xor(az, o); }
    const float n = (float)max(p1 - p0, 1);
    d[0] = ci[0] - ax / n; d[1] = ci[1] - ay / n; d[2] = ci[2] - az / n;
}

// The COM of the graph's new centers (pharmacodiff.py:413-429) and its removal from centers and protein, for the whole workgroup:
// per-thread sums, the xor butterfly per wave, ((r0 + r1) + (r2 + r3)) / n -- the one reduction order of every form of a step.
// cen: the node of the thread's center (m: its new coordinates, still in registers) or -1; pa: protein row ia, requested by the
// caller before its first wait; the rows beyond it at stride 256
__device__ __forceinline__ void com_remove(float4* xn, const int cen, const float m[3], const int ncen, const int ia, const int p1, float4 pa) {
    __shared__ float com[3];
    __shared__ float red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (cen >= 0) { sx += m[0]; sy += m[1]; sz += m[2]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); sz += __shfl_xor(sz, o); }
    if (lane == 0) { red[wave][0] = sx; red[wave][1] = sy; red[wave][2] = sz; }
    __syncthreads();
    if (tid == 0) {
        const float n = (float)max(ncen, 1);
        for (int c = 0; c < 3; ++c) com[c] = (ncen > 0) ? (((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) / n) : 0.f;
    }
    __syncthreads();
    const float cx = com[0], cy = com[1], cz = com[2];
    if (cen >= 0) xn[cen] = make_float4(m[0] - cx, m[1] - cy, m[2] - cz, 0.f);
    if (ia < p1) { pa.x -= cx; pa.y -= cy; pa.z -= cz; xn[ia] = pa; }
    for (int i = ia + 256; i < p1; i += 256) {
        float4 x = xn[i];
        x.x -= cx; x.y -= cy; x.z -= cz;
        xn[i] = x;
    }
}

// ---------------------------------------------------------------------------------------------
// The moves.  A move says what the skeleton requests for it -- STATE (the center's state row), NOISE, EPS (the network's outputs),
// flags(), an auxiliary row per center (aux_x / aux_h: history, pins or seed; nullptr: not read, zeros stand in), FRAME (D[g]: not
// needed; reduced from frame() = c_init; given in frame() = D as k_guide_grad left it), SNAP (the features also go to h_snap_out),
// BUILD_FORM (k_step_build is instantiated for it) -- and computes, for the thread's center f: coords() the three new coordinates, feat() one new feature (feat_begin() once in front).
// z / nz / e / a: the value's state, noise, output and auxiliary entry; d: D[g].  Every expression keeps one rounding per operation
// (pf_feat_update, pf_ms_update, pf_noised_value, pf_guide_shift*: contraction off)
// ---------------------------------------------------------------------------------------------
enum { PF_FRAME_NONE, PF_FRAME_REDUCE, PF_FRAME_GIVEN };
struct MoveBase {
    static constexpr bool STATE = true, NOISE = true, EPS = true, SNAP = false, BUILD_FORM = true;
    static constexpr int FRAME = PF_FRAME_NONE;
    static constexpr int NH = 8;                        // features per row held in registers (pharm_nf is 6 in every shipped configuration); the rest: after the wait
    __device__ const float* frame() const { return nullptr; }
    __device__ const int* flags() const { return nullptr; }
    __device__ const float* aux_x(int, int) const { return nullptr; }
    __device__ const float* aux_h(int, int) const { return nullptr; }
    __device__ float feat_begin(const StepParams&, int) const { return 1.0f; }
};
// z_s = mu + sigma * noise (sample_p_zs_given_zt, pharmacodiff.py:397-426)
struct MovePlain : MoveBase {
    __device__ void coords(const StepParams& p, int, int, const float* z, const float* nz, const float* e, const float*, const float*, float* m) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = pf_feat_update(z[c], e[c], nz[c], p.a_ts, p.var, p.sigma, p.ep_zt, p.ep_pred, p.ep_coord);
    }
    __device__ float feat(const StepParams& p, int, int, int, float z, float nz, float e, float, float) const {
        return pf_feat_update(z, e, nz, p.a_ts, p.var, p.sigma, p.ep_zt, p.ep_pred, p.ep_feat);
    }
};
// Multistep move (pf_denoise_step_ms): the linear combination pf_ms_update, no noise.  The thread that reads an element's output
// also stores it as that element's history, for the next multistep move; the history is read only where c1 != 0
struct MoveMs : MoveBase {
    static constexpr bool NOISE = false;
    MsParams q;
    __device__ const float* aux_x(int f, int nf) const { return q.c1_x != 0.f ? q.hist + (size_t)f * (3 + nf) : nullptr; }
    __device__ const float* aux_h(int f, int nf) const { return q.c1_h != 0.f ? q.hist + (size_t)f * (3 + nf) + 3 : nullptr; }
    __device__ void coords(const StepParams& p, int f, int, const float* z, const float*, const float* e, const float* a, const float*, float* m) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m[c] = pf_ms_update(z[c], e[c], a[c], q.cz_x, q.c0_x, q.c1_x, q.c1_x != 0.f);
            q.hist[(size_t)f * (3 + p.nf) + c] = e[c];
        }
    }
    __device__ float feat(const StepParams& p, int f, int k, int, float z, float, float e, float a, float) const {
        q.hist[(size_t)f * (3 + p.nf) + 3 + k] = e;
        return pf_ms_update(z, e, a, q.cz_h, q.c0_h, q.c1_h, q.c1_h != 0.f);
    }
};
// Pinned centers (replacement conditioning, pf_denoise_step_pinned): the plain move with two selects in front of its stores.  A
// center whose position is given (flag bit 0) becomes the given position noised to this step's level with the step's own noise draw
// (its posterior sample is discarded); likewise a center whose feature row is given (bit 1).  Given positions are in the caller's
// frame: sampler frame = caller's frame - D[g]
struct MovePinned : MoveBase {
    static constexpr int FRAME = PF_FRAME_REDUCE;
    static constexpr int NH = 6;                        // (four rows per center: with 8 the move alone would not keep 8 waves per SIMD)
    PinParams q;
    __device__ const float* frame() const { return q.com_init; }
    __device__ const int* flags() const { return q.flags; }
    __device__ const float* aux_x(int f, int) const { return q.pin_x + (size_t)f * 3; }
    __device__ const float* aux_h(int f, int nf) const { return q.pin_h + (size_t)f * nf; }
    __device__ void coords(const StepParams& p, int, int flag, const float* z, const float* nz, const float* e, const float* a, const float* d, float* m) const {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            m[c] = (flag & 1) ? pf_noised_value(a[c] - d[c], nz[c], q.alpha_s, q.sigma_s)
                              : pf_feat_update(z[c], e[c], nz[c], p.a_ts, p.var, p.sigma, p.ep_zt, p.ep_pred, p.ep_coord);
    }
    __device__ float pin_feat(int flag, float a, float nz, float fr) const { return (flag & 2) ? pf_noised_value(a / q.feat_norm, nz, q.alpha_s, q.sigma_s) : fr; }
    __device__ float feat(const StepParams& p, int, int, int flag, float z, float nz, float e, float a, float) const {
        return pin_feat(flag, a, nz, pf_feat_update(z, e, nz, p.a_ts, p.var, p.sigma, p.ep_zt, p.ep_pred, p.ep_feat));
    }
};
// Guided (pf_denoise_step_guided): the pinned move with one more input -- the guided step's shift is taken off a free center's
// p(z_s | z_t) value in front of the selects, and D[g] is the one k_guide_grad left (the same reduction of the same rows, which
// nobody has moved in between).  FEAT (type guidance, pf_guide_types_next): the feature rows are guided too -- a free center's
// feature row loses shift_h in front of the `flag & 2` select, as its position loses the shift in front of `flag & 1`
template <bool FEAT>
struct MoveGuided : MovePinned {
    static constexpr int FRAME = PF_FRAME_GIVEN;
    static constexpr bool BUILD_FORM = false;           // (the guided step's training forward builds its own edges: the move alone)
    GuideShiftParams gs;
    GuideFeatParams gf;                                 // FEAT only
    __device__ const float* frame() const { return gs.D; }
    __device__ void coords(const StepParams& p, int f, int flag, const float* z, const float* nz, const float* e, const float* a, const float* d, float* m) const {
        MovePinned::coords(p, f, flag, z, nz, e, a, d, m);
        float gr[3], sh[3];
        pf_guide_shift(gs.g0 + (size_t)f * 3, gs.jx + (size_t)f * 3, gs.alpha_t, gs.sigma_t, p.ep_coord, p.sigma, gs.scale, gs.clip, gr, sh);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gs.grad[(size_t)f * 3 + c] = gr[c]; gs.shift[(size_t)f * 3 + c] = sh[c];
            if (!(flag & 1)) m[c] -= sh[c];             // (a position-pinned center ignores its shift)
        }
    }
    __device__ float feat_begin(const StepParams& p, int f) const {      // the clip's factor of this row
        if constexpr (!FEAT) return 1.0f;
        else return pf_guide_shift_h(gf.g0_h + (size_t)f * p.nf, gf.jh + (size_t)f * p.nf, p.nf, gs.alpha_t, gs.sigma_t, p.ep_coord, p.ep_feat, p.sigma,
                                     gf.scale, gf.clip, gf.grad_h + (size_t)f * p.nf, gf.shift_h + (size_t)f * p.nf);
    }
    __device__ float feat(const StepParams& p, int f, int k, int flag, float z, float nz, float e, float a, float hf) const {
        float fr = pf_feat_update(z, e, nz, p.a_ts, p.var, p.sigma, p.ep_zt, p.ep_pred, p.ep_feat);
        if constexpr (FEAT) {
            float sh = gf.shift_h[(size_t)f * p.nf + k];                // (this thread's own store, unclipped)
            if (hf != 1.0f) { sh *= hf; gf.shift_h[(size_t)f * p.nf + k] = sh; }
            fr -= sh;
        }
        return pin_feat(flag, a, nz, fr);
    }
};
// Resampling jump of a pinned run (pf_renoise_step): the whole state of graph g goes from level b back up to level a > b,
// z_a = alpha_{a|b} * z_b + sigma_{a|b} * noise, for every center -- pinned or free -- and for coordinates and feature rows alike.
// Nothing of the caller's frame enters
struct MoveRenoise : MoveBase {
    static constexpr bool EPS = false;
    RenoiseParams q;
    __device__ void coords(const StepParams&, int, int, const float* z, const float* nz, const float*, const float*, const float*, float* m) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = pf_noised_value(z[c], nz[c], q.alpha_ts, q.sigma_ts);
    }
    __device__ float feat(const StepParams&, int, int, int, float z, float nz, float, float, float) const { return pf_noised_value(z, nz, q.alpha_ts, q.sigma_ts); }
};
// Seeded begin (pf_sample_seed_next): in place of "state := noise0", every center of graph g becomes the caller's seed noised forward
// to level a, z_a = alpha_a * seed + sigma_a * noise0 -- the pinned move's arithmetic with every center flagged 3.  Seed positions are in
// the caller's frame.  The state's own rows are not read: whatever the previous run left in them is dead.  The feature rows also go to
// the center-hoist snapshot (h_snap_out) the first step's hoist workgroups read
struct MoveSeed : MoveBase {
    static constexpr bool STATE = false, EPS = false, SNAP = true;
    static constexpr int FRAME = PF_FRAME_REDUCE;
    SeedParams q;
    __device__ const float* frame() const { return q.com_init; }
    __device__ const float* aux_x(int f, int) const { return q.seed_x + (size_t)f * 3; }
    __device__ const float* aux_h(int f, int nf) const { return q.seed_h + (size_t)f * nf; }
    __device__ void coords(const StepParams&, int, int, const float*, const float* nz, const float*, const float* a, const float* d, float* m) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = pf_noised_value(a[c] - d[c], nz[c], q.alpha_a, q.sigma_a);
    }
    __device__ float feat(const StepParams&, int, int, int, float, float nz, float, float a, float) const { return pf_noised_value(a / q.feat_norm, nz, q.alpha_a, q.sigma_a); }
};

// ---------------------------------------------------------------------------------------------
// The skeleton: graph g's move, for the whole workgroup (256 threads)
// ---------------------------------------------------------------------------------------------
struct MoveRows { const float* nz; const float* er; const float* ax; const float* ar; float* hr; };      // center f's rows: noise, eps_h, aux, state features
template <class M>
__device__ __forceinline__ MoveRows move_rows(const StepParams& p, const M& mv, const int f) {
    return {p.noise + (size_t)f * (3 + p.nf), p.eps_h + (size_t)f * p.nf, mv.aux_x(f, p.nf), mv.aux_h(f, p.nf), p.pharm_h + (size_t)f * p.nf};
}
template <class M>
__device__ __forceinline__ void step_move_body(const StepParams& p, const M& mv, const int g) {
    constexpr int NH = M::NH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = p.pharm_ptr[g], f1 = p.pharm_ptr[g + 1];
    const int p0 = p.prot_ptr[g], p1 = p.prot_ptr[g + 1];
    const int ia = p0 + tid, nf = p.nf;                 // the thread's first atom
    int f = f0 + tid;                                   // ... and its center (wave 0: at most 64 per graph)
    const bool own = f < f1;
    // ---- every row the thread needs, requested before the first wait
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ia < p1) pa = p.xn[ia];                         // wave 0's also serve frame_offset; shifted by com_remove
    float ci[3] = {0.f, 0.f, 0.f};                      // c_init, or D[g] as it was left (uniform: scalar registers)
    if (M::FRAME != PF_FRAME_NONE) for (int c = 0; c < 3; ++c) ci[c] = mv.frame()[3 * g + c];
    float z[3] = {0.f, 0.f, 0.f}, nx[3] = {0.f, 0.f, 0.f}, e[3] = {0.f, 0.f, 0.f}, a[3] = {0.f, 0.f, 0.f};
    float zh[NH], nh[NH], eh[NH], ah[NH];               // the first NH features of each row
#pragma unroll
    for (int j = 0; j < NH; ++j) { zh[j] = 0.f; nh[j] = 0.f; eh[j] = 0.f; ah[j] = 0.f; }
    int flag = 0;
    if (own) {
        const MoveRows r = move_rows(p, mv, f);
        if (M::STATE) { const float4 xa = p.xn[p.Np_tot + f]; z[0] = xa.x; z[1] = xa.y; z[2] = xa.z; }
        if (mv.flags()) flag = mv.flags()[f];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (M::NOISE) nx[c] = r.nz[c];
            if (M::EPS) e[c] = p.eps_x[(size_t)f * 3 + c];
            if (r.ax) a[c] = r.ax[c];
        }
#pragma unroll
        for (int j = 0; j < NH; ++j) if (j < nf) {
            if (M::STATE) zh[j] = r.hr[j];
            if (M::NOISE) nh[j] = r.nz[3 + j];
            if (M::EPS) eh[j] = r.er[j];
            if (r.ar) ah[j] = r.ar[j];
        }
    }
    {   // an empty asm the compiler cannot move the loads across, as in pf_stepbuild.h.  It also hands f back as a new value: what
        // follows computes its addresses again, so none of the loads' address registers stays live next to the loaded rows
        float pin = (((z[0] + z[1]) + (z[2] + nx[0])) + ((nx[1] + nx[2]) + (e[0] + e[1]))) + ((e[2] + a[0]) + (a[1] + a[2]));
#pragma unroll
        for (int j = 0; j < NH; ++j) pin += (zh[j] + nh[j]) + (eh[j] + ah[j]);
        asm volatile("" : "+v"(f) : "v"(pin), "v"(pa.x), "v"(flag), "s"(ci[0]), "s"(ci[1]), "s"(ci[2]) : "memory");
    }
    // ---- D[g]
    float d[3] = {ci[0], ci[1], ci[2]};
    if (M::FRAME == PF_FRAME_REDUCE && wave == 0) frame_offset(p.xn, p0, p1, lane, pa, ci, d);
    // ---- the center's new values: coordinates into registers, features stored
    float m[3] = {0.f, 0.f, 0.f};
    if (own) {
        const MoveRows r = move_rows(p, mv, f);
        mv.coords(p, f, flag, z, nx, e, a, d, m);
        const float hf = mv.feat_begin(p, f);
        float* const hs = (M::SNAP && p.h_snap_out) ? p.h_snap_out + (size_t)f * nf : nullptr;
        auto put = [&](const int k, const float zv, const float nv, const float ev, const float av) {
            const float v = mv.feat(p, f, k, flag, zv, nv, ev, av, hf);
            r.hr[k] = v;
            if (hs) hs[k] = v;
        };
#pragma unroll
        for (int j = 0; j < NH; ++j) if (j < nf) put(j, zh[j], nh[j], eh[j], ah[j]);
        for (int k = NH; k < nf; ++k) put(k, M::STATE ? r.hr[k] : 0.f, M::NOISE ? r.nz[3 + k] : 0.f, M::EPS ? r.er[k] : 0.f, r.ar ? r.ar[k] : 0.f);
    }
    // ---- the COM of the new centers, off centers and protein
    com_remove(p.xn, own ? p.Np_tot + f : -1, m, f1 - f0, ia, p1, pa);
}
