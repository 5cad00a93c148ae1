// rt_probe_batch.h — the host half of rt_debug_closest_hits (rt_probe.cpp) without HIP: the checks of
// the caller's rays and the batch laid out as the band the launch traces. Plain C++, so the sanitizer
// build (tests/native/Makefile `sanitize`) runs exactly this code.
#pragma once

#include <cstdint>
#include <vector>

namespace rt {
namespace probe {

constexpr uint32_t kProbeBandW = 512;          // texels per band row: a multiple of the 8x8 tile
constexpr uint32_t kProbeMaxRays = 1u << 24;   // band height below 65536

// rays6: n rays {ox, oy, oz, vx, vy, vz}, n in [1, kProbeMaxRays]. Returns 0, or the index + 1 of
// the first ray refused: a value that is not finite, a direction without a nonzero component, or an
// origin whose |o|^2 overflows. On success `rays` holds *band_h rows of kProbeBandW rays, the last
// row padded with copies of ray 0 (every texel of the band is traced), and *cam_r the largest |o|
// of the batch, in the binary32 operations fill_trace computes a camera's distance with.
uint32_t stage_batch(const float* rays6, uint32_t n, std::vector<float>& rays, uint32_t* band_h, float* cam_r);

}  // namespace probe
}  // namespace rt
