// rt_temporal.hip — the kernels of rt_temporal_accumulate_device and rt_temporal_reproject_device
// (include/rt_mi355x.h): one thread per texel, blocks of kTileW x kTileH texels as
// the denoisers'. The in-place kernel reads no neighbour, so it updates the state planes where they
// lie; the reprojected kernel fetches its history from up to four texels around the place its motion
// vector names, so it reads one set of planes and writes another. A texel moves float4 only: it loads
// A (and B), feat0, feat1, HA (and HB) and HG (per tap, and the motion vector, when reprojected), and
// stores HA (and HB), HG, out_a (and out_b), one 16-byte access per lane each, beside the optional
// 4-byte sample count, rgba8 and history length. Two instantiations each, one accumulator and two;
// the optional outputs are branches on launch-uniform pointers. Every operation is one correctly
// rounded binary32 + - x / in the order the contract writes it (the library is built with
// -ffp-contract=off, never -ffast-math).
#include <hip/hip_runtime.h>

#include "rt_denoise_host.h"
#include "rt_device_math.h"
#include "rt_temporal.h"

using namespace rtd;

namespace {

constexpr uint32_t kTileW = rt::denoise::kTileW, kTileH = rt::denoise::kTileH;

struct Rgb {
    float x, y, z;
};

// One accumulator's history H = (e.rgb, n) and its frame sum S of h samples: e' by the contract.
// `a` is the demodulation albedo, alpha = 1 / n'; h == 0 is a frame without a measurement.
__device__ __forceinline__ Rgb integrate(const float4& S, const float4& H, const Rgb& a, uint32_t h, float hf, bool valid,
                                         float alpha) {
    if (h == 0u) return valid ? Rgb{H.x, H.y, H.z} : Rgb{0.0f, 0.0f, 0.0f};
    const float ex = (S.x / hf) / a.x, ey = (S.y / hf) / a.y, ez = (S.z / hf) / a.z;
    if (!valid) return Rgb{ex, ey, ez};
    return Rgb{H.x + alpha * (ex - H.x), H.y + alpha * (ey - H.y), H.z + alpha * (ez - H.z)};
}

// The filters' feature stop between the guide (nrm, z) and a history guide HG.
__device__ __forceinline__ float feature_stop(const rt::TemporalParams& K, float nx, float ny, float nz, float z,
                                              const float4& HG) {
    const float dnx = nx - HG.x, dny = ny - HG.y, dnz = nz - HG.z;
    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
    const float dz = (z - HG.w) / (z + 1.0f);
    return (1.0f + K.k_normal * dn2) * (1.0f + K.k_depth * (dz * dz));
}

// One tap of the reprojected history: its weight, its texel (the caller's own where it does not
// count, so that its loads stay inside the planes) and whether it lies in the band.
struct Tap {
    float w;
    size_t q;
    bool in;
};

}  // namespace

template <bool TWO>
__global__ __launch_bounds__(kTileW* kTileH) void rt_temporal_kernel(const rt::TemporalParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const float4 A = reinterpret_cast<const float4*>(K.accum_a)[i];
    const float4 f0 = reinterpret_cast<const float4*>(K.feat0)[i];
    const float4 f1 = reinterpret_cast<const float4*>(K.feat1)[i];
    const float4 HA = reinterpret_cast<const float4*>(K.ha)[i];
    const float4 HG = reinterpret_cast<const float4*>(K.hg)[i];
    const uint32_t h = K.sample_count ? K.sample_count[i] : K.spp;
    const float hf = float(h), F = K.feature_samples;
    const Rgb a = {f0.x / F + 0x1p-6f, f0.y / F + 0x1p-6f, f0.z / F + 0x1p-6f};
    const float4 g = make_float4(f1.x / F, f1.y / F, f1.z / F, f1.w / F);
    // the guide against the history's: the filters' feature stop
    const float dnx = g.x - HG.x, dny = g.y - HG.y, dnz = g.z - HG.z;
    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
    const float dz = (g.w - HG.w) / (g.w + 1.0f);
    const float stop = (1.0f + K.k_normal * dn2) * (1.0f + K.k_depth * (dz * dz));
    const bool valid = HA.w > 0.0f && stop < 2.0f;
    float n;
    if (h == 0u) n = valid ? HA.w : 0.0f;
    else if (valid) n = __builtin_fminf(HA.w + 1.0f, K.max_history);
    else n = 1.0f;
    const float alpha = 1.0f / n;   // unused for h == 0
    const Rgb ea = integrate(A, HA, a, h, hf, valid, alpha);
    reinterpret_cast<float4*>(K.ha)[i] = make_float4(ea.x, ea.y, ea.z, n);
    reinterpret_cast<float4*>(K.hg)[i] = g;
    reinterpret_cast<float4*>(K.out_a)[i] = make_float4(ea.x * a.x, ea.y * a.y, ea.z * a.z, 1.0f);
    Rgb m = {ea.x * a.x, ea.y * a.y, ea.z * a.z};
    if constexpr (TWO) {
        const float4 B = reinterpret_cast<const float4*>(K.accum_b)[i];
        const float4 HB = reinterpret_cast<const float4*>(K.hb)[i];
        const Rgb eb = integrate(B, HB, a, h, hf, valid, alpha);
        reinterpret_cast<float4*>(K.hb)[i] = make_float4(eb.x, eb.y, eb.z, n);
        reinterpret_cast<float4*>(K.out_b)[i] = make_float4(eb.x * a.x, eb.y * a.y, eb.z * a.z, 1.0f);
        m = Rgb{((ea.x + eb.x) * 0.5f) * a.x, ((ea.y + eb.y) * 0.5f) * a.y, ((ea.z + eb.z) * 0.5f) * a.z};
    }
    if (K.out_rgba8) {   // rt_tonemap_kernel at spp 1
        const uint32_t r8 = unorm8(__builtin_sqrtf(m.x / 1.0f));
        const uint32_t g8 = unorm8(__builtin_sqrtf(m.y / 1.0f));
        const uint32_t b8 = unorm8(__builtin_sqrtf(m.z / 1.0f));
        K.out_rgba8[i] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
    }
    if (K.history_len) K.history_len[i] = uint32_t(n);
}

// The reprojected call: the kernel above with the history (HA, HB) of a texel replaced by the
// weighted mean of the taps that count, and `valid` by "a tap counts". The first tap's loads are
// issued for every texel; the other three only where a wave holds a texel off the snap (a static
// texel has one tap), all nine together.
template <bool TWO>
__global__ __launch_bounds__(kTileW* kTileH) void rt_temporal_reproject_kernel(const rt::TemporalReprojectParams R) {
    const rt::TemporalParams& K = R.T;
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const float4 A = reinterpret_cast<const float4*>(K.accum_a)[i];
    const float4 f0 = reinterpret_cast<const float4*>(K.feat0)[i];
    const float4 f1 = reinterpret_cast<const float4*>(K.feat1)[i];
    const float4 mv = reinterpret_cast<const float4*>(R.motion)[i];
    const float4* __restrict__ ha_src = reinterpret_cast<const float4*>(R.ha_src);
    const float4* __restrict__ hb_src = reinterpret_cast<const float4*>(R.hb_src);
    const float4* __restrict__ hg_src = reinterpret_cast<const float4*>(R.hg_src);
    const uint32_t h = K.sample_count ? K.sample_count[i] : K.spp;
    const float hf = float(h), F = K.feature_samples;
    const Rgb a = {f0.x / F + 0x1p-6f, f0.y / F + 0x1p-6f, f0.z / F + 0x1p-6f};
    const float4 g = make_float4(f1.x / F, f1.y / F, f1.z / F, f1.w / F);
    // where the history lies: texel centres are at integer + 0.5
    const float bx = mv.x - 0.5f, by = mv.y - 0.5f;
    const float jx = __builtin_floorf(bx + 0.5f), jy = __builtin_floorf(by + 0.5f);
    const bool snap = __builtin_fabsf(bx - jx) <= 0x1p-6f && __builtin_fabsf(by - jy) <= 0x1p-6f;
    const float ix = __builtin_floorf(bx), iy = __builtin_floorf(by);
    const float fx = bx - ix, fy = by - iy;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const bool ok = mv.w > 0.0f;
    const float ze = g.w + mv.z;
    const float Wf = float(K.band_w), Hf = float(K.band_h);
    auto make_tap = [&](float tx, float ty, float w) -> Tap {
        const bool in = ok && w > 0.0f && tx >= 0.0f && tx < Wf && ty >= 0.0f && ty < Hf;
        const uint32_t qx = uint32_t(in ? tx : 0.0f), qy = uint32_t(in ? ty : 0.0f);
        return Tap{w, in ? size_t(qy) * K.band_w + qx : i, in};
    };
    float Wt = 0.0f, sn = 0.0f;
    Rgb sa = {0.0f, 0.0f, 0.0f}, sb = {0.0f, 0.0f, 0.0f};
    auto add_tap = [&](const Tap& t, const float4& HA, const float4& HG, const float4& HB) {
        const float stop = feature_stop(K, g.x, g.y, g.z, ze, HG);
        const bool counts = t.in && HA.w > 0.0f && stop < 2.0f;
        Wt = Wt + (counts ? t.w : 0.0f);
        sa.x = sa.x + (counts ? t.w * HA.x : 0.0f);
        sa.y = sa.y + (counts ? t.w * HA.y : 0.0f);
        sa.z = sa.z + (counts ? t.w * HA.z : 0.0f);
        sn = sn + (counts ? t.w * HA.w : 0.0f);
        if constexpr (TWO) {
            sb.x = sb.x + (counts ? t.w * HB.x : 0.0f);
            sb.y = sb.y + (counts ? t.w * HB.y : 0.0f);
            sb.z = sb.z + (counts ? t.w * HB.z : 0.0f);
        }
    };
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    {
        const Tap t0 = snap ? make_tap(jx, jy, 1.0f) : make_tap(ix, iy, gx * gy);
        const float4 HA = ha_src[t0.q], HG = hg_src[t0.q];
        float4 HB = zero4;
        if constexpr (TWO) HB = hb_src[t0.q];
        add_tap(t0, HA, HG, HB);
    }
    if (!snap) {
        const Tap t1 = make_tap(ix + 1.0f, iy, fx * gy);
        const Tap t2 = make_tap(ix, iy + 1.0f, gx * fy);
        const Tap t3 = make_tap(ix + 1.0f, iy + 1.0f, fx * fy);
        const float4 HA1 = ha_src[t1.q], HG1 = hg_src[t1.q];
        const float4 HA2 = ha_src[t2.q], HG2 = hg_src[t2.q];
        const float4 HA3 = ha_src[t3.q], HG3 = hg_src[t3.q];
        float4 HB1 = zero4, HB2 = zero4, HB3 = zero4;
        if constexpr (TWO) {
            HB1 = hb_src[t1.q];
            HB2 = hb_src[t2.q];
            HB3 = hb_src[t3.q];
        }
        add_tap(t1, HA1, HG1, HB1);
        add_tap(t2, HA2, HG2, HB2);
        add_tap(t3, HA3, HG3, HB3);
    }
    const bool valid = Wt > 0.0f;
    const float4 HA = make_float4(sa.x / Wt, sa.y / Wt, sa.z / Wt, sn / Wt);   // read where valid alone
    float n;
    if (h == 0u) n = valid ? HA.w : 0.0f;
    else if (valid) n = __builtin_fminf(HA.w + 1.0f, K.max_history);
    else n = 1.0f;
    const float alpha = 1.0f / n;   // unused for h == 0
    const Rgb ea = integrate(A, HA, a, h, hf, valid, alpha);
    reinterpret_cast<float4*>(K.ha)[i] = make_float4(ea.x, ea.y, ea.z, n);
    reinterpret_cast<float4*>(K.hg)[i] = g;
    reinterpret_cast<float4*>(K.out_a)[i] = make_float4(ea.x * a.x, ea.y * a.y, ea.z * a.z, 1.0f);
    Rgb m = {ea.x * a.x, ea.y * a.y, ea.z * a.z};
    if constexpr (TWO) {
        const float4 B = reinterpret_cast<const float4*>(K.accum_b)[i];
        const float4 HB = make_float4(sb.x / Wt, sb.y / Wt, sb.z / Wt, HA.w);
        const Rgb eb = integrate(B, HB, a, h, hf, valid, alpha);
        reinterpret_cast<float4*>(K.hb)[i] = make_float4(eb.x, eb.y, eb.z, n);
        reinterpret_cast<float4*>(K.out_b)[i] = make_float4(eb.x * a.x, eb.y * a.y, eb.z * a.z, 1.0f);
        m = Rgb{((ea.x + eb.x) * 0.5f) * a.x, ((ea.y + eb.y) * 0.5f) * a.y, ((ea.z + eb.z) * 0.5f) * a.z};
    }
    if (K.out_rgba8) {   // rt_tonemap_kernel at spp 1
        const uint32_t r8 = unorm8(__builtin_sqrtf(m.x / 1.0f));
        const uint32_t g8 = unorm8(__builtin_sqrtf(m.y / 1.0f));
        const uint32_t b8 = unorm8(__builtin_sqrtf(m.z / 1.0f));
        K.out_rgba8[i] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
    }
    if (K.history_len) K.history_len[i] = uint32_t(n);
}

namespace rt {

hipError_t launch_temporal(const TemporalParams& K, hipStream_t st) {
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (!K.accum_a || !K.feat0 || !K.feat1 || !K.ha || !K.hg || !K.out_a) return hipErrorInvalidValue;
    if (K.accum_b && (!K.hb || !K.out_b)) return hipErrorInvalidValue;
    const void* fn = K.accum_b ? reinterpret_cast<const void*>(rt_temporal_kernel<true>)
                               : reinterpret_cast<const void*>(rt_temporal_kernel<false>);
    void* args[] = {const_cast<TemporalParams*>(&K)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(fn, grid, dim3(kTileW * kTileH), args, 0, st);
}

hipError_t launch_temporal_reproject(const TemporalReprojectParams& R, hipStream_t st) {
    const TemporalParams& K = R.T;
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (!K.accum_a || !K.feat0 || !K.feat1 || !K.ha || !K.hg || !K.out_a || !R.motion || !R.ha_src || !R.hg_src)
        return hipErrorInvalidValue;
    if (K.accum_b && (!K.hb || !K.out_b || !R.hb_src)) return hipErrorInvalidValue;
    if (R.ha_src == K.ha || R.hg_src == K.hg) return hipErrorInvalidValue;   // taps read what neighbours write
    const void* fn = K.accum_b ? reinterpret_cast<const void*>(rt_temporal_reproject_kernel<true>)
                               : reinterpret_cast<const void*>(rt_temporal_reproject_kernel<false>);
    void* args[] = {const_cast<TemporalReprojectParams*>(&R)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(fn, grid, dim3(kTileW * kTileH), args, 0, st);
}

}  // namespace rt
