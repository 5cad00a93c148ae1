// rt_temporal_host.h — the host half of the temporal stage (rt_temporal_create,
// rt_temporal_accumulate_device; rt_features.cpp) without HIP: the checks of the call's parameters,
// their defaults, and the sizes of a state's planes. Plain C++, so the sanitizer build
// (tests/test_temporal_host.py) runs exactly this code. The kernel is rt_temporal.hip; the contract
// is include/rt_mi355x.h and DESIGN.md §3.1.3.
#pragma once

#include <cstdint>

#include "rt_denoise_host.h"

namespace rt {
namespace temporal {

constexpr uint32_t kMinHistory = 2, kMaxHistory = 65535;   // n is held as a float: exact to 2^24
constexpr uint32_t kPlanes = 3;                            // HA, HB, HG: one float4 per texel each
constexpr rt_temporal_params kDefaults = {8u, 4.0f, 16.0f, 0u};

// rt_temporal_check. *p: the parameters in force (the defaults for params == nullptr). The size and
// feature-sample limits are rt_denoise_check's. Returns RT_OK or RT_ERR_INVALID_ARGUMENT with *err a
// static message that names the field.
int check(const rt_temporal_params* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples,
          rt_temporal_params* p, const char** err);

// The band of a state (rt_temporal_create): both sides within 1 .. 65535.
int check_band(uint32_t band_w, uint32_t band_h, const char** err);

// Texels of a plane, the floats from one plane to the next, and the bytes of a state's one allocation.
uint64_t plane_texels(uint32_t band_w, uint32_t band_h);
uint64_t plane_floats(uint32_t band_w, uint32_t band_h);
uint64_t state_bytes(uint32_t band_w, uint32_t band_h);

}  // namespace temporal
}  // namespace rt
