// rt_temporal.hip — the kernel of rt_temporal_accumulate_device (include/rt_mi355x.h, DESIGN.md
// §3.1.3): one thread per texel, blocks of kTileW x kTileH texels as the denoisers', no neighbour
// read, so the state planes are updated in place. A texel moves float4 only: it loads A (and B),
// feat0, feat1, HA (and HB) and HG, and stores HA (and HB), HG, out_a (and out_b), one 16-byte
// access per lane each, beside the optional 4-byte sample count, rgba8 and history length. Two
// instantiations, one accumulator and two; the optional outputs are branches on launch-uniform
// pointers. Every operation is one correctly rounded binary32 + - x / in the order the contract
// writes it (the library is built with -ffp-contract=off, never -ffast-math).
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

}  // namespace rt
