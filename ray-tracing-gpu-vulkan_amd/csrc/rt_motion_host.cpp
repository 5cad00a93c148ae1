// rt_motion_host.cpp — rt_motion_host.h.
#include "rt_motion_host.h"

#include <cmath>

#include "rt_denoise_host.h"

namespace rt {
namespace motion {

namespace {

struct F3 { float x, y, z; };
inline F3 f3(float x, float y, float z) { return F3{x, y, z}; }
inline F3 operator+(F3 a, F3 b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline F3 operator-(F3 a, F3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline float dot3(F3 a, F3 b) { return std::fma(a.z, b.z, std::fma(a.y, b.y, a.x * b.x)); }
inline F3 unit(F3 v) {
    float len = std::sqrt(dot3(v, v));
    float inv = 1.0f / len;
    return f3(v.x * inv, v.y * inv, v.z * inv);
}
inline F3 cross3(F3 a, F3 b) {
    return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline void put(float* d, F3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
inline F3 get(const float* s) { return f3(s[0], s[1], s[2]); }

}  // namespace

void camera(const RenderCallInfo& rci, Camera* out) {
    const float fov = 25.0f, focus = 10.0f;   // shader.rgen:29 (the aperture is the constant 0)
    const F3 up = f3(0.0f, 1.0f, 0.0f);
    const F3 from = f3(rci.camera_pos.x, rci.camera_pos.y, rci.camera_pos.z);
    const F3 at = from + f3(rci.camera_dir.x, rci.camera_dir.y, rci.camera_dir.z);
    const float sx = float(rci.image_size.x), sy = float(rci.image_size.y);
    const float aspect = sx / sy;
    const float half = (fov * 0.017453292519943295f) / 2.0f;
    const float vh = float(std::tan(double(half))) * 2.0f;
    const float vw = aspect * vh;
    const F3 fwd = unit(at - from);
    const F3 right = unit(cross3(up, fwd));
    const F3 cup = unit(cross3(fwd, right));
    const F3 hor = f3(vw * right.x * focus, vw * right.y * focus, vw * right.z * focus);
    const F3 ver = f3(vh * cup.x * focus, vh * cup.y * focus, vh * cup.z * focus);
    const F3 ulc = ((from - f3(hor.x / 2.0f, hor.y / 2.0f, hor.z / 2.0f)) +
                    f3(ver.x / 2.0f, ver.y / 2.0f, ver.z / 2.0f)) +
                   f3(fwd.x * focus, fwd.y * focus, fwd.z * focus);
    put(out->lf, from);
    put(out->hor, hor);
    put(out->ver, ver);
    put(out->ulc, ulc);
    out->size_x = sx;
    out->size_y = sy;
    out->inv_size_x = 1.0 / double(sx);
    out->inv_size_y = 1.0 / double(sy);
}

void projection(const Camera& prev, Projection* out) {
    const F3 lf = get(prev.lf), hor = get(prev.hor), ver = get(prev.ver);
    const F3 u = get(prev.ulc) - lf;
    const F3 wn = cross3(hor, ver);
    put(out->lf, lf);
    put(out->hor, hor);
    put(out->ver, ver);
    put(out->u, u);
    put(out->wn, wn);
    out->k = dot3(u, wn);
    out->ihh = 1.0f / dot3(hor, hor);
    out->ivv = 1.0f / dot3(ver, ver);
}

int check_band(uint32_t band_w, uint32_t band_h, const char** err) {
    *err = "";
    if (band_w == 0u || band_h == 0u || band_w > 65535u || band_h > 65535u) {
        *err = "rt_motion_create: band width and height must be within 1 .. 65535";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

int check(uint32_t band_w, uint32_t band_h, const RenderCallInfo* rci, const RenderCallInfo* prev, const char** err) {
    rt_denoise unused;
    if (int rc = denoise::check(nullptr, band_w, band_h, 1u, &unused, err)) return rc;
    if (!rci) {
        *err = "rt_motion: rci is NULL";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (rci->image_size.x == 0u || rci->image_size.y == 0u) {
        *err = "rt_motion: image_size is zero";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (prev && (prev->image_size.x != rci->image_size.x || prev->image_size.y != rci->image_size.y)) {
        *err = "rt_motion: the previous frame's image_size differs from this frame's";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

uint64_t texels(uint32_t band_w, uint32_t band_h) { return uint64_t(band_w) * band_h; }

uint64_t ray_bytes(uint32_t band_w, uint32_t band_h) { return texels(band_w, band_h) * kRayFloats * sizeof(float); }

uint64_t hit_bytes(uint32_t band_w, uint32_t band_h) { return texels(band_w, band_h) * kHitWords * sizeof(uint32_t); }

}  // namespace motion
}  // namespace rt
