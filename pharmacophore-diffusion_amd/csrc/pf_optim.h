// The guarded optimiser step (pf_adam_step_guarded, pf_debug_optim_step): parameters of its three launches, shared by the
// kernels (pf_optim.hip) and the host entries (pf_host.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// one workgroup of PFO_THREADS reduces / updates one contiguous chunk of PFO_CHUNK floats (pf_debug_optim_chunk)
constexpr int PFO_CHUNK = 4096;
constexpr int PFO_THREADS = 256;

// the caller-owned state block (include/pfdyn.h: PF_OPTIM_STATE_BYTES = 64, layout documented there); bc1 / bc2_sqrt are the
// hand-over of k_optim_finalize to the k_adam_guarded launch behind it
struct OptimState {
    long long applied, skipped;
    float norm, coef;
    int finite;
    float bc1, bc2_sqrt;
    int reserved[7];
};
static_assert(sizeof(OptimState) == 64, "PF_OPTIM_STATE_BYTES");

struct OptimParams {
    float* p; const float* g; float* m; float* v;
    float* ema;                              // or NULL
    float* mirror;                           // the handle's own flat copy, or NULL
    size_t n;
    float lr, b1, b2, eps, wd, grad_scale;
    int clip_mode; float clip, ema_decay;
    double* partials;                        // [ceil(n / PFO_CHUNK)]
    OptimState* state;
};

void pfk_optim_step(const OptimParams& p, hipStream_t s);
void pfk_optim_state_init(OptimState* state, long long applied, hipStream_t s);
