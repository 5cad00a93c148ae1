// rt_denoise_var.h — the kernel argument of one launch of the variance-guided denoise (a prefilter
// pass or an iteration) and its launcher (rt_denoise_var.hip), as rt_features.cpp calls it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct DenoiseVarParams {
    uint32_t band_w, band_h;
    uint32_t step;                  // 1 << index of the pass or iteration
    uint32_t half_spp;              // the uniform half sample count (half_count == nullptr)
    float feature_samples;          // float(F)
    float k_normal, k_depth, k_color;
    // the caller's buffers: read by the first launch (the prologue); feat0 also by the last
    const float* accum_a;
    const float* accum_b;
    const uint32_t* half_count;     // optional
    const float* feat0;
    const float* feat1;
    // the context's band buffers (float4 per texel): E = (e, v) of the previous launch, the guide
    // plane G = (nrm, z) the first launch stored, this launch's E
    const float* src;
    const float* guide;
    float* guide_out;               // first launch (when it is not the last too)
    float* dst;
    // the last iteration (the epilogue)
    float* out_mean;                // optional
    uint32_t* out_rgba8;
};

// prefilter: a feature-only pass over the variance, else an iteration; first / last: the launch
// folds the prologue / the epilogue (only an iteration is ever last); lds_step: its step when it
// stages its taps in LDS (1, 2 or 4), 0 for taps from global memory.
hipError_t launch_denoise_var(const DenoiseVarParams& K, bool prefilter, bool first, bool last, uint32_t lds_step,
                              hipStream_t st);

}  // namespace rt
