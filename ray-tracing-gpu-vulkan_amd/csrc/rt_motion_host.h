// rt_motion_host.h — the host half of the motion pass (rt_motion_create, rt_render_motion_device;
// rt_motion.cpp) without HIP: the checks of the call's arguments, the pinhole camera of a
// RenderCallInfo as the frames derive it, the constants of the motion kernel from the previous
// frame's camera, and the sizes of a motion object's planes. Plain C++, so the sanitizer build
// (tests/test_motion_host.py) runs exactly this code. The kernels are rt_motion_kernels.hip; the contract is
// include/rt_mi355x.h and DESIGN.md §3.1.3.
#pragma once

#include <cstdint>

#include "../../include/rt_mi355x.h"

namespace rt {
namespace motion {

constexpr uint32_t kRayFloats = 6;     // a texel's ray: origin, then the direction before normalisation
constexpr uint32_t kHitWords = 2;      // a texel's answer: the winning sphere or 0xffffffff, the bits of t

// The pinhole camera of a frame: rt_api.cpp fill_camera's expressions (shader.rgen:29, 48-49,
// 92-105), operation for operation, so that the rays of the motion pass start where the frame's do.
struct Camera {
    float lf[3], hor[3], ver[3], ulc[3];
    float size_x, size_y;
    double inv_size_x, inv_size_y;
};
void camera(const RenderCallInfo& rci, Camera* out);

// What the motion kernel reads of the previous frame's camera, binary32, computed once per launch:
//     u = ulc' - lf';  wn = cross(hor', ver');  k = dot(u, wn)
//     ihh = 1 / dot(hor', hor');  ivv = 1 / dot(ver', ver')
// dot is fma(a.z, b.z, fma(a.y, b.y, a.x b.x)), cross is (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
// a.x b.y - a.y b.x), every product and difference rounded.
struct Projection {
    float lf[3], hor[3], ver[3], u[3], wn[3];
    float k, ihh, ivv;
};
void projection(const Camera& prev, Projection* out);

// The band of a motion object (rt_motion_create): both sides within 1 .. 65535.
int check_band(uint32_t band_w, uint32_t band_h, const char** err);

// rt_motion_check: the band as rt_denoise_check takes it, rci not NULL with a nonzero image size,
// and a previous frame (NULL: none) of the same image size.
// Returns RT_OK or RT_ERR_INVALID_ARGUMENT with *err a static message that names the field.
int check(uint32_t band_w, uint32_t band_h, const RenderCallInfo* rci, const RenderCallInfo* prev, const char** err);

// Texels of a band and the bytes of a motion object's ray and answer planes.
uint64_t texels(uint32_t band_w, uint32_t band_h);
uint64_t ray_bytes(uint32_t band_w, uint32_t band_h);
uint64_t hit_bytes(uint32_t band_w, uint32_t band_h);

}  // namespace motion
}  // namespace rt
