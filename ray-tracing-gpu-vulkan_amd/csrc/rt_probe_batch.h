// rt_probe_batch.h — the host halves of rt_debug_closest_hits (rt_probe.cpp) and rt_debug_scatter
// (rt_probe_scatter.cpp) without HIP: the checks of the caller's rays and the batch laid out as the
// band the launch traces; the checks of a batch of hits to shade. Plain C++, so the sanitizer
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

// The argument checks of rt_debug_scatter on n cases, n in [1, kProbeMaxRays]: returns 0, or the index
// + 1 of the first case refused: a ray value or a t that is not finite, a direction without a nonzero
// component, or ids[i] >= n_spheres.
uint32_t check_scatter_batch(const float* rays6, const uint32_t* ids, const float* t, uint32_t n, uint32_t n_spheres);
// The record forms of rt_debug_scatter: the scene's global arrays, or the static LDS table of
// rt::kRecStatic (rec_capacity) spheres. False for an unknown form and for form 1 on a larger scene.
constexpr uint32_t kScatterFormGlobal = 0, kScatterFormRec = 1;
bool scatter_form_ok(uint32_t form, uint32_t n_spheres, uint32_t rec_capacity);

}  // namespace probe
}  // namespace rt
