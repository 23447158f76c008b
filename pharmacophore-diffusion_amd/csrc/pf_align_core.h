// The arithmetic of one (query, entry) pair of pf_pharm_align (include/pfdyn.h, "pharmacophore alignment"), written
// once for the device (pf_align.hip) and the host (tests/align_check.cpp runs a whole pair serially without a GPU): the rotation
// solve, a seed's transform, the typed overlap, the matched count, one refinement round, and the refinement loop with its outputs.
// Plain fp32, one rounding per operation (FP contraction off), no memory but the caller's arrays.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) && defined(__HIP__)
#define PF_ALIGN_HD __host__ __device__ __forceinline__
#else
#define PF_ALIGN_HD inline
#endif

#define PF_ALIGN_JACOBI_SWEEPS 6                // cyclic sweeps of the symmetric 4 x 4 matrix: converged in fp32 after 4 to 5

// a pair as the kernels see it: nq <= 16 query centers x [nq][3], t [nq]; nl <= 32 entry centers y [nl][3], u [nl];
// mask [nl]: bit p of mask[q] is set when t_p == u_q
struct AlignPairView {
    int nq, nl;
    const float* x; const int* t;
    const float* y; const int* u;
    const unsigned* mask;
};

// x' = R (y - yc) + xc: centered, so that a translation of tens of angstroms costs no digits of the rotated part
struct AlignXf { float R[9], yc[3], xc[3]; };

// a seed's key: its place in the enumeration order (i, j, k, a, b, c), i < j < k < 16 and a, b, c < 32 -- integer order = that order
PF_ALIGN_HD int align_key(int i, int j, int k, int a, int b, int c) { return (i << 23) | (j << 19) | (k << 15) | (a << 10) | (b << 5) | c; }

// The proper rotation (det +1) R that minimises sum w |R (y - yc) - (x - xc)|^2, in Horn's form: S[a * 3 + b] = sum w (y - yc)_a (x - xc)_b;
// the unit quaternion of R is the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix N(S), found by a fixed
// number of cyclic Jacobi sweeps (every rotation unrolled: the matrix and the vectors stay in registers).  A quaternion always
// gives a proper rotation: a mirror image is never produced.
PF_ALIGN_HD void align_rotation(const float S[9], float R[9]) {
#pragma clang fp contract(off)
    float A[4][4], V[4][4];
    const float Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    A[0][0] = (Sxx + Syy) + Szz;  A[0][1] = Syz - Szy;          A[0][2] = Szx - Sxz;           A[0][3] = Sxy - Syx;
    A[1][1] = (Sxx - Syy) - Szz;  A[1][2] = Sxy + Syx;          A[1][3] = Szx + Sxz;
    A[2][2] = (Syy - Sxx) - Szz;  A[2][3] = Syz + Szy;
    A[3][3] = (Szz - Sxx) - Syy;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { if (c < r) A[r][c] = A[c][r]; V[r][c] = r == c ? 1.f : 0.f; }
#pragma unroll 1
    for (int sweep = 0; sweep < PF_ALIGN_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const float apq = A[p][q];
                const float theta = (A[q][q] - A[p][p]) / (2.f * apq);
                // t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)); apq == 0 (theta inf or nan) or theta^2 overflowing: no rotation
                float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
                if (!(apq != 0.f) || !(t == t)) t = 0.f;
                const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = 0.f; A[q][p] = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r != p && r != q) {
                        const float arp = A[r][p], arq = A[r][q];
                        const float np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                        A[r][p] = np_; A[p][r] = np_; A[r][q] = nq_; A[q][r] = nq_;
                    }
                    const float vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq; V[r][q] = s * vrp + c * vrq;
                }
            }
    }
    float best = A[0][0], q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for (int m = 1; m < 4; ++m)
        if (A[m][m] > best) { best = A[m][m]; q0 = V[0][m]; qx = V[1][m]; qy = V[2][m]; qz = V[3][m]; }
    const float n = 1.f / sqrtf((q0 * q0 + qx * qx) + (qy * qy + qz * qz));
    q0 = q0 * n; qx = qx * n; qy = qy * n; qz = qz * n;
    const float ww = q0 * q0, xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const float xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = q0 * qx, wy = q0 * qy, wz = q0 * qz;
    R[0] = (ww + xx) - (yy + zz);  R[1] = 2.f * (xy - wz);          R[2] = 2.f * (xz + wy);
    R[3] = 2.f * (xy + wz);          R[4] = (ww + yy) - (xx + zz);  R[5] = 2.f * (yz - wx);
    R[6] = 2.f * (xz - wy);          R[7] = 2.f * (yz + wx);          R[8] = (ww + zz) - (xx + yy);
}

PF_ALIGN_HD void align_apply(const AlignXf& T, const float* y, float out[3]) {
#pragma clang fp contract(off)
    const float d0 = y[0] - T.yc[0], d1 = y[1] - T.yc[1], d2 = y[2] - T.yc[2];
    out[0] = ((T.R[0] * d0 + T.R[1] * d1) + T.R[2] * d2) + T.xc[0];
    out[1] = ((T.R[3] * d0 + T.R[4] * d1) + T.R[5] * d2) + T.xc[1];
    out[2] = ((T.R[6] * d0 + T.R[7] * d1) + T.R[8] * d2) + T.xc[2];
}

// the transform of a seed: the least-squares proper rotation and translation over its three correspondences
PF_ALIGN_HD void align_seed_xf(const AlignPairView& P, int key, AlignXf& T) {
#pragma clang fp contract(off)
    const int qi[3] = {(key >> 23) & 15, (key >> 19) & 15, (key >> 15) & 15}, li[3] = {(key >> 10) & 31, (key >> 5) & 31, key & 31};
    const float third = 1.f / 3.f;
    for (int e = 0; e < 3; ++e) {
        T.xc[e] = ((P.x[qi[0] * 3 + e] + P.x[qi[1] * 3 + e]) + P.x[qi[2] * 3 + e]) * third;
        T.yc[e] = ((P.y[li[0] * 3 + e] + P.y[li[1] * 3 + e]) + P.y[li[2] * 3 + e]) * third;
    }
    float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float dy[3], dx[3];
        for (int e = 0; e < 3; ++e) { dy[e] = P.y[li[m] * 3 + e] - T.yc[e]; dx[e] = P.x[qi[m] * 3 + e] - T.xc[e]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[a * 3 + b] = S[a * 3 + b] + dy[a] * dx[b];
    }
    align_rotation(S, T.R);
}

// O = sum_q ( sum_{p: t_p == u_q} exp(-|x_p - (R y_q + s)|^2 / (2 sigma^2)) ): the inner sums p ascending, then q ascending
PF_ALIGN_HD float align_overlap(const AlignPairView& P, const AlignXf& T, float inv_2s2) {
#pragma clang fp contract(off)
    float O = 0.f;
    for (int q = 0; q < P.nl; ++q) {
        const unsigned m = P.mask[q];
        if (!m) continue;
        float r[3];
        align_apply(T, P.y + q * 3, r);
        float o = 0.f;
        for (int p = 0; p < P.nq; ++p) {
            if (!((m >> p) & 1u)) continue;
            const float dx = P.x[p * 3] - r[0], dy = P.x[p * 3 + 1] - r[1], dz = P.x[p * 3 + 2] - r[2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            o = o + expf(-(d2 * inv_2s2));
        }
        O = O + o;
    }
    return O;
}

// the self overlap of one pharmacophore (the same order: inner sums over the same-type centers, then over the centers)
PF_ALIGN_HD float align_self_overlap(int n, const float* x, const int* t, float inv_2s2) {
#pragma clang fp contract(off)
    float O = 0.f;
    for (int q = 0; q < n; ++q) {
        float o = 0.f;
        for (int p = 0; p < n; ++p) {
            if (t[p] != t[q]) continue;
            const float dx = x[p * 3] - x[q * 3], dy = x[p * 3 + 1] - x[q * 3 + 1], dz = x[p * 3 + 2] - x[q * 3 + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            o = o + expf(-(d2 * inv_2s2));
        }
        O = O + o;
    }
    return O;
}

// the number of query centers with a same-type entry center within the tolerance (<=) after the transform
PF_ALIGN_HD int align_matched(const AlignPairView& P, const AlignXf& T, float tol2) {
#pragma clang fp contract(off)
    unsigned hit = 0u;
    for (int q = 0; q < P.nl; ++q) {
        const unsigned m = P.mask[q];
        if (!m) continue;
        float r[3];
        align_apply(T, P.y + q * 3, r);
        for (int p = 0; p < P.nq; ++p) {
            if (!((m >> p) & 1u)) continue;
            const float dx = P.x[p * 3] - r[0], dy = P.x[p * 3 + 1] - r[1], dz = P.x[p * 3 + 2] - r[2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= tol2) hit |= 1u << p;
        }
    }
    int n = 0;
    for (int p = 0; p < P.nq; ++p) n += (hit >> p) & 1u;
    return n;
}

// One refinement round: weights at the transform `cur`, the weighted least-squares transform over all same-type pairs into `next`.
// false when the weights sum to nothing a transform could be made of (the refinement then stops)
PF_ALIGN_HD bool align_refine_round(const AlignPairView& P, const AlignXf& cur, float inv_2s2, AlignXf& next) {
#pragma clang fp contract(off)
    float W = 0.f, sx[3] = {0.f, 0.f, 0.f}, sy[3] = {0.f, 0.f, 0.f};
    for (int q = 0; q < P.nl; ++q) {
        const unsigned m = P.mask[q];
        if (!m) continue;
        float r[3];
        align_apply(cur, P.y + q * 3, r);
        for (int p = 0; p < P.nq; ++p) {
            if (!((m >> p) & 1u)) continue;
            const float dx = P.x[p * 3] - r[0], dy = P.x[p * 3 + 1] - r[1], dz = P.x[p * 3 + 2] - r[2];
            const float w = expf(-(((dx * dx + dy * dy) + dz * dz) * inv_2s2));
            W = W + w;
            for (int e = 0; e < 3; ++e) { sx[e] = sx[e] + w * P.x[p * 3 + e]; sy[e] = sy[e] + w * P.y[q * 3 + e]; }
        }
    }
    if (!(W > 0.f) || !(W < INFINITY)) return false;
    for (int e = 0; e < 3; ++e) { next.xc[e] = sx[e] / W; next.yc[e] = sy[e] / W; }
    float S[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < P.nl; ++q) {
        const unsigned m = P.mask[q];
        if (!m) continue;
        float r[3], dyv[3];
        align_apply(cur, P.y + q * 3, r);
        for (int e = 0; e < 3; ++e) dyv[e] = P.y[q * 3 + e] - next.yc[e];
        for (int p = 0; p < P.nq; ++p) {
            if (!((m >> p) & 1u)) continue;
            const float dx = P.x[p * 3] - r[0], dy = P.x[p * 3 + 1] - r[1], dz = P.x[p * 3 + 2] - r[2];
            const float w = expf(-(((dx * dx + dy * dy) + dz * dz) * inv_2s2));
            float dxv[3];
            for (int e = 0; e < 3; ++e) dxv[e] = w * (P.x[p * 3 + e] - next.xc[e]);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) S[a * 3 + b] = S[a * 3 + b] + dyv[a] * dxv[b];
        }
    }
    align_rotation(S, next.R);
    return true;
}

struct AlignResult { float sim; int matched; float xf[12]; };

// From the best seed (overlap O at transform T) to the pair's outputs: up to `refine` rounds, each accepted when the overlap does
// not fall; the similarity against the two self overlaps; the matched count; R row-major and s = xc - R yc
PF_ALIGN_HD void align_finish(const AlignPairView& P, AlignXf T, float O, int refine, float inv_2s2, float tol2, float o_qq, float o_ll,
                              AlignResult& out) {
#pragma clang fp contract(off)
    for (int r = 0; r < refine; ++r) {
        AlignXf N;
        if (!align_refine_round(P, T, inv_2s2, N)) break;
        const float O2 = align_overlap(P, N, inv_2s2);
        if (!(O2 >= O)) break;
        T = N; O = O2;
    }
    out.sim = fminf(O / ((o_qq + o_ll) - O), 1.0f);
    out.matched = align_matched(P, T, tol2);
    for (int e = 0; e < 9; ++e) out.xf[e] = T.R[e];
    for (int e = 0; e < 3; ++e)
        out.xf[9 + e] = T.xc[e] - ((T.R[e * 3] * T.yc[0] + T.R[e * 3 + 1] * T.yc[1]) + T.R[e * 3 + 2] * T.yc[2]);
}

// the seed filters on one candidate (types, the three distance differences, the entry triplet's area); dq_*: the query triplet's
PF_ALIGN_HD float align_dist(const float* a, const float* b) {
#pragma clang fp contract(off)
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}
PF_ALIGN_HD float align_area(const float* o, const float* p, const float* q) {            // |(p - o) x (q - o)|
#pragma clang fp contract(off)
    const float ux = p[0] - o[0], uy = p[1] - o[1], uz = p[2] - o[2], vx = q[0] - o[0], vy = q[1] - o[1], vz = q[2] - o[2];
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return sqrtf((cx * cx + cy * cy) + cz * cz);
}

// A whole pair, one seed after the other: what k_align_pairs computes with its lanes, in the order of the definition.  Host code
// (tests/align_check.cpp); mask: scratch of nl words.  Returns the number of seeds
inline int align_pair_serial(int nq, const float* x, const int* t, int nl, const float* y, const int* u, unsigned* mask, float inv_2s2,
                             float tol2, float seed_tol, float min_area, int refine, AlignResult& out) {
    for (int q = 0; q < nl; ++q) {
        mask[q] = 0u;
        for (int p = 0; p < nq; ++p) mask[q] |= (t[p] == u[q]) ? (1u << p) : 0u;
    }
    const AlignPairView P{nq, nl, x, t, y, u, mask};
    float best_o = -1.f;
    int best_key = 0x7fffffff, n_seeds = 0;
    for (int i = 0; i < nq; ++i) for (int j = i + 1; j < nq; ++j) for (int k = j + 1; k < nq; ++k) {
        if (!(align_area(x + i * 3, x + j * 3, x + k * 3) >= min_area)) continue;
        const float d_ij = align_dist(x + i * 3, x + j * 3), d_ik = align_dist(x + i * 3, x + k * 3), d_jk = align_dist(x + j * 3, x + k * 3);
        for (int a = 0; a < nl; ++a) for (int b = 0; b < nl; ++b) for (int c = 0; c < nl; ++c) {
            if (a == b || a == c || b == c || u[a] != t[i] || u[b] != t[j] || u[c] != t[k]) continue;
            if (!(std::fabs(d_ij - align_dist(y + a * 3, y + b * 3)) <= seed_tol) || !(std::fabs(d_ik - align_dist(y + a * 3, y + c * 3)) <= seed_tol) ||
                !(std::fabs(d_jk - align_dist(y + b * 3, y + c * 3)) <= seed_tol) || !(align_area(y + a * 3, y + b * 3, y + c * 3) >= min_area))
                continue;
            ++n_seeds;
            const int key = align_key(i, j, k, a, b, c);
            AlignXf T;
            align_seed_xf(P, key, T);
            const float o = align_overlap(P, T, inv_2s2);
            if (o > best_o || (o == best_o && key < best_key)) { best_o = o; best_key = key; }
        }
    }
    if (n_seeds > 0 && best_o >= 0.f) {
        AlignXf T;
        align_seed_xf(P, best_key, T);
        align_finish(P, T, best_o, refine, inv_2s2, tol2, align_self_overlap(nq, x, t, inv_2s2), align_self_overlap(nl, y, u, inv_2s2), out);
    } else {
        out.sim = 0.f; out.matched = 0;
        for (int e = 0; e < 12; ++e) out.xf[e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
    }
    return n_seeds;
}
