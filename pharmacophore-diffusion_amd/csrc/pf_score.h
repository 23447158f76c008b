// pf_score: the parameters of one noise level of a scoring call (k_score_prepare / k_score_eval, pf_score.hip), shared by the
// kernels and the host entry (pf_host.cpp: pf_score)
#pragma once
#include <hip/hip_runtime.h>

struct ScoreParams {
    int B, Np, nf, t_int, remove_com;
    int first;                               // the call's first level: score is stored, not added to
    float feat_norm, w_pos, w_feat;
    const int* prot_ptr; const int* pharm_ptr;
    const float* prot_x0;                    // [Np][3] as bound
    const float* x0; const float* h0;        // the candidates: clean centers [Nf][3] (caller's frame), raw feature one-hots [Nf][nf]
    const float* noise;                      // this level's row [Nf][3 + nf], x columns first (the sampler's layout)
    const float* alpha_tab; const float* sigma_tab;      // [T + 1]
    float4* xn; float* pharm_h;              // the dynamics' input state
    const float* dyn_h; const float* dyn_x;  // the dynamics' outputs
    float* score;                            // [B][2]
    float* terms;                            // this level's [B][4] = pos, feat, err, hits; or NULL
};
