// rt_temporal.h — the kernel argument of rt_temporal_accumulate_device's one launch and its launcher
// (rt_temporal.hip), as rt_features.cpp calls it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct TemporalParams {
    uint32_t band_w, band_h;
    uint32_t spp;                   // the uniform sample count (sample_count == nullptr)
    float feature_samples;          // float(F)
    float k_normal, k_depth;
    float max_history;              // float(max_history), exact
    // the caller's buffers
    const float* accum_a;
    const float* accum_b;           // null: one accumulator (hb and out_b unused)
    const uint32_t* sample_count;   // optional
    const float* feat0;
    const float* feat1;
    // the state's planes (float4 per texel), updated in place
    float* ha;                      // (eA.rgb, n)
    float* hb;                      // (eB.rgb, n)
    float* hg;                      // (nrm.xyz, z)
    // outputs
    float* out_a;
    float* out_b;
    uint32_t* out_rgba8;            // optional
    uint32_t* history_len;          // optional
};

// rt_temporal_reproject_device's one launch: T as above with ha / hb / hg the plane set the call
// WRITES, and the set it reads its history taps from, which must be another one.
struct TemporalReprojectParams {
    TemporalParams T;
    const float* motion;            // float4 per texel (sx, sy, dzm, ok)
    const float* ha_src;
    const float* hb_src;
    const float* hg_src;
};

// One launch of one thread per texel; the two-accumulator instantiation when K.accum_b is set.
hipError_t launch_temporal(const TemporalParams& K, hipStream_t st);
hipError_t launch_temporal_reproject(const TemporalReprojectParams& K, hipStream_t st);

}  // namespace rt
