// rt_denoise.h — the kernel argument of one denoise iteration and its launcher (rt_denoise.hip),
// as rt_features.cpp calls it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct DenoiseParams {
    uint32_t band_w, band_h;
    uint32_t step;                  // 1 << iteration
    uint32_t spp;                   // the uniform sample count (sample_count == nullptr)
    float feature_samples;          // float(F)
    float k_normal, k_depth;
    float k_color;                  // k_color * 4^iteration
    // the caller's buffers: read by the first iteration (the prologue); feat0 also by the last
    const float* accum;
    const uint32_t* sample_count;   // optional
    const float* feat0;
    const float* feat1;
    // the context's band buffers (float4 per texel): E of the previous iteration, the guide plane
    // G = (nrm, z) the first iteration stored, this iteration's E
    const float* src;
    const float* guide;
    float* guide_out;               // first iteration (when it is not the last too)
    float* dst;
    // the last iteration (the epilogue)
    float* out_mean;                // optional
    uint32_t* out_rgba8;
};

// first / last: the iteration folds the prologue / the epilogue; lds_step: its step when it stages
// its taps in LDS (1, 2 or 4), 0 for taps from global memory.
hipError_t launch_denoise(const DenoiseParams& K, bool first, bool last, uint32_t lds_step, hipStream_t st);

}  // namespace rt
