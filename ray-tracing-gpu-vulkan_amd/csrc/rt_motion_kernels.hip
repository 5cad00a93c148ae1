// rt_motion_kernels.hip — the two kernels of rt_render_motion_device (include/rt_mi355x.h)
// on either side of the MODE_PROBE trace: one thread per texel, blocks of kTileW x kTileH texels as
// the denoisers'. The first writes the pinhole ray through each texel's centre (camera_ray's
// expressions without the jitter draws), the second turns the trace's (winner, t) into the texel's
// place in the previous frame's image. Every operation is one correctly rounded binary32 operation
// in the order the contract writes it (the library is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_denoise_host.h"
#include "rt_device_math.h"
#include "rt_motion.h"

using namespace rtd;

namespace {

constexpr uint32_t kTileW = rt::denoise::kTileW, kTileH = rt::denoise::kTileH;

__device__ __forceinline__ V3 v3a(const float* p) { return v3(p[0], p[1], p[2]); }

__device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

}  // namespace

__global__ __launch_bounds__(kTileW* kTileH) void rt_motion_rays_kernel(const rt::MotionRayParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const uint32_t gx = K.off_x + x, gy = K.off_y + y;
    const float ux = float(double(float(gx) + 0.5f) * K.inv_size_x);
    const float uy = float(double(float(gy) + 0.5f) * K.inv_size_y);
    const V3 lf = v3a(K.lf);
    const V3 to = sub(add(v3a(K.ulc), scale(ux, v3a(K.hor))), scale(uy, v3a(K.ver)));
    const V3 v = sub(to, lf);
    float* r = K.rays + 6u * i;
    r[0] = lf.x; r[1] = lf.y; r[2] = lf.z;
    r[3] = v.x; r[4] = v.y; r[5] = v.z;
}

__global__ __launch_bounds__(kTileW* kTileH) void rt_motion_kernel(const rt::MotionParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const float* q = K.rays + 6u * i;
    const V3 o = v3(q[0], q[1], q[2]);
    const V3 d = normalize(v3(q[3], q[4], q[5]));
    const uint32_t id = K.hits[2u * i];
    const float t = __uint_as_float(K.hits[2u * i + 1u]);
    const bool hit = id != 0xffffffffu;
    const bool moved = K.same_count != 0u && id < K.n_spheres;   // (a winner is always below n_spheres)
    V3 r = d;   // a miss: the sky is a point at infinity
    if (hit) {
        V3 p = v3(__builtin_fmaf(t, d.x, o.x), __builtin_fmaf(t, d.y, o.y), __builtin_fmaf(t, d.z, o.z));
        if (moved) {   // otherwise the previous frame's ids mean other spheres
            const float4 cn = K.geom_now[id], cp = K.geom_prev[id];
            p = add(sub(p, v3(cn.x, cn.y, cn.z)), v3(cp.x, cp.y, cp.z));
        }
        r = sub(p, v3a(K.lf));
    }
    const V3 hor = v3a(K.hor), ver = v3a(K.ver);
    const float den = dot(r, v3a(K.wn));
    const float s = K.k / den;
    const V3 rel = sub(scale(s, r), v3a(K.u));
    const float sx = ((dot(rel, hor) * K.ihh) * K.size_x) - K.off_x;
    const float sy = ((-(dot(rel, ver) * K.ivv)) * K.size_y) - K.off_y;
    const float dzm = hit ? sqrt_cr(dot(r, r)) - t : 0.0f;
    const bool ok = den > 0.0f && finite(sx) && finite(sy) && (!hit || moved);
    reinterpret_cast<float4*>(K.motion)[i] = make_float4(sx, sy, dzm, ok ? 1.0f : 0.0f);
}

namespace rt {

hipError_t launch_motion_rays(const MotionRayParams& K, hipStream_t st) {
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (!K.rays) return hipErrorInvalidValue;
    void* args[] = {const_cast<MotionRayParams*>(&K)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(reinterpret_cast<const void*>(rt_motion_rays_kernel), grid, dim3(kTileW * kTileH), args, 0, st);
}

hipError_t launch_motion(const MotionParams& K, hipStream_t st) {
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (!K.rays || !K.hits || !K.motion) return hipErrorInvalidValue;
    if (K.same_count && (!K.geom_now || !K.geom_prev)) return hipErrorInvalidValue;
    void* args[] = {const_cast<MotionParams*>(&K)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(reinterpret_cast<const void*>(rt_motion_kernel), grid, dim3(kTileW * kTileH), args, 0, st);
}

}  // namespace rt
