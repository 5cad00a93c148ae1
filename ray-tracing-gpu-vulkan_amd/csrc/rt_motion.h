// rt_motion.h — the kernel arguments of the motion pass's two own launches and their launchers
// (rt_motion_kernels.hip), as rt_motion.cpp calls them: the rays through the texel centres ahead of the
// MODE_PROBE trace, and the motion plane from its answers behind it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct MotionRayParams {
    uint32_t band_w, band_h;
    uint32_t off_x, off_y;          // rci->offset
    float lf[3], hor[3], ver[3], ulc[3];
    double inv_size_x, inv_size_y;
    float* rays;                    // band_w * band_h x {o.xyz, v.xyz}
};

struct MotionParams {
    uint32_t band_w, band_h;
    uint32_t n_spheres;             // of this frame's scene
    uint32_t same_count;            // the previous frame holds as many spheres as this one
    float size_x, size_y;           // float(image_size)
    float off_x, off_y;             // float(rci->offset)
    // the previous frame's camera (rt_motion_host.h Projection)
    float lf[3], hor[3], ver[3], u[3], wn[3];
    float k, ihh, ivv;
    const float* rays;
    const uint32_t* hits;           // per texel {winner or 0xffffffff, bits of t}
    const float4* geom_now;         // per sphere id, xyz the centre
    const float4* geom_prev;
    float* motion;                  // float4 per texel (sx, sy, dzm, ok)
};

// One launch each of one thread per texel.
hipError_t launch_motion_rays(const MotionRayParams& K, hipStream_t st);
hipError_t launch_motion(const MotionParams& K, hipStream_t st);

}  // namespace rt
