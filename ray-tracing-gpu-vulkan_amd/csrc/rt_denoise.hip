// rt_denoise.hip — the kernels of rt_denoise_device (include/rt_mi355x.h): an
// edge-avoiding a-trous filter of the frame's mean colour, demodulated by the first-hit albedo and
// guided by the first-hit normal and depth. One kernel per iteration, one thread per texel, blocks
// of kTileW x kTileH texels. The first iteration computes its inputs from the caller's buffers (the
// prologue: c, a, e_0, nrm, z) and stores the guide plane; the last multiplies the albedo back and
// tonemaps (the epilogue). Every operation is one correctly rounded binary32 + - x / in the order
// the contract writes it (the library is built with -ffp-contract=off, never -ffast-math).
//
// A texel's filter state is two float4: E = (e.rgb, 0) and G = (nrm.xyz, z). Iterations of small
// step stage the E and G of their tile and its halo of 2 step texels in LDS once, where the 25 taps
// of neighbouring texels overlap (LDS_STEP > 0); the others read their taps from global memory.
// Both forms run the same tap loop on the same values, so they give the same bits.
#include <hip/hip_runtime.h>

#include "rt_denoise.h"
#include "rt_denoise_host.h"
#include "rt_device_math.h"

using namespace rtd;

namespace {

constexpr uint32_t kTileW = rt::denoise::kTileW, kTileH = rt::denoise::kTileH;

struct Texel {
    float4 e, g;
};

// The prologue for texel i: c = accum.rgb / n (0 for n = 0), a = feat0.rgb / F, e_0 = c / (a + 2^-6),
// nrm = feat1.xyz / F, z = feat1.w / F.
__device__ __forceinline__ Texel prologue(const rt::DenoiseParams& K, size_t i) {
    const float4 acc = reinterpret_cast<const float4*>(K.accum)[i];
    const float4 f0 = reinterpret_cast<const float4*>(K.feat0)[i];
    const float4 f1 = reinterpret_cast<const float4*>(K.feat1)[i];
    const uint32_t n = K.sample_count ? K.sample_count[i] : K.spp;
    const float fn = float(n), F = K.feature_samples;
    const float cx = n ? acc.x / fn : 0.0f, cy = n ? acc.y / fn : 0.0f, cz = n ? acc.z / fn : 0.0f;
    const float ax = f0.x / F + 0x1p-6f, ay = f0.y / F + 0x1p-6f, az = f0.z / F + 0x1p-6f;
    Texel t;
    t.e = make_float4(cx / ax, cy / ay, cz / az, 0.0f);
    t.g = make_float4(f1.x / F, f1.y / F, f1.z / F, f1.w / F);
    return t;
}

template <bool FIRST>
__device__ __forceinline__ Texel load_texel(const rt::DenoiseParams& K, size_t i) {
    if constexpr (FIRST) {
        return prologue(K, i);
    } else {
        Texel t;
        t.e = reinterpret_cast<const float4*>(K.src)[i];
        t.g = reinterpret_cast<const float4*>(K.guide)[i];
        return t;
    }
}

// One tap of weight kk = K[|dy|] K[|dx|] at texel q, seen from p.
__device__ __forceinline__ void tap(const rt::DenoiseParams& K, const Texel& p, const Texel& q, float kk, float& nx,
                                    float& ny, float& nz, float& den) {
    const float dnx = p.g.x - q.g.x, dny = p.g.y - q.g.y, dnz = p.g.z - q.g.z;
    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
    const float dz = (p.g.w - q.g.w) / (p.g.w + 1.0f);
    const float dex = p.e.x - q.e.x, dey = p.e.y - q.e.y, dez = p.e.z - q.e.z;
    const float de2 = (dex * dex + dey * dey) + dez * dez;
    const float x = ((1.0f + K.k_normal * dn2) * (1.0f + K.k_depth * (dz * dz))) * (1.0f + K.k_color * de2);
    const float w = kk / (x * x);
    nx += w * q.e.x;
    ny += w * q.e.y;
    nz += w * q.e.z;
    den += w;
}

__device__ __forceinline__ float kernel_weight(int d) {   // the B3 spline {1, 4, 6, 4, 1} / 16
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// e_{i+1}(p) stored, or with LAST the epilogue: mean = e (a + 2^-6), (mean, 1) and its rgba8.
template <bool FIRST, bool LAST>
__device__ __forceinline__ void store_texel(const rt::DenoiseParams& K, size_t i, const Texel& p, float ex, float ey,
                                            float ez) {
    if constexpr (FIRST && !LAST) reinterpret_cast<float4*>(K.guide_out)[i] = p.g;
    if constexpr (LAST) {
        const float4 f0 = reinterpret_cast<const float4*>(K.feat0)[i];
        const float F = K.feature_samples;
        const float mx = ex * (f0.x / F + 0x1p-6f), my = ey * (f0.y / F + 0x1p-6f), mz = ez * (f0.z / F + 0x1p-6f);
        if (K.out_mean) reinterpret_cast<float4*>(K.out_mean)[i] = make_float4(mx, my, mz, 1.0f);
        // rt_tonemap_kernel at spp 1
        const uint32_t r8 = unorm8(__builtin_sqrtf(mx / 1.0f));
        const uint32_t g8 = unorm8(__builtin_sqrtf(my / 1.0f));
        const uint32_t b8 = unorm8(__builtin_sqrtf(mz / 1.0f));
        K.out_rgba8[i] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
    } else {
        reinterpret_cast<float4*>(K.dst)[i] = make_float4(ex, ey, ez, 0.0f);
    }
}

}  // namespace

// Taps from global memory (the large steps; any step in the forced form of the tests).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_plain_kernel(const rt::DenoiseParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const Texel p = load_texel<FIRST>(K, i);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, den = 0.0f;
    const int step = int(K.step), w = int(K.band_w), h = int(K.band_h);
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = int(y) + dy * step;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = int(x) + dx * step;
            if (qx < 0 || qx >= w) continue;
            const Texel q = load_texel<FIRST>(K, size_t(qy) * K.band_w + uint32_t(qx));
            tap(K, p, q, kernel_weight(dy) * kernel_weight(dx), nx, ny, nz, den);
        }
    }
    store_texel<FIRST, LAST>(K, i, p, nx / den, ny / den, nz / den);
}

// Taps from LDS: the block stages the texels [x0 - 2 STEP, x0 + kTileW + 2 STEP) x [y0 - 2 STEP,
// y0 + kTileH + 2 STEP) that lie in the band (with FIRST, their prologue once per texel instead of
// once per tap), then every thread reads its 25 taps there. 32 B per staged texel.
template <bool FIRST, bool LAST, int STEP>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_lds_kernel(const rt::DenoiseParams K) {
    constexpr int HALO = 2 * STEP, SW = int(kTileW) + 2 * HALO, SH = int(kTileH) + 2 * HALO;
    __shared__ float4 s_e[SW * SH];
    __shared__ float4 s_g[SW * SH];
    const int x0 = int(blockIdx.x * kTileW) - HALO, y0 = int(blockIdx.y * kTileH) - HALO;
    const int w = int(K.band_w), h = int(K.band_h);
    for (int s = int(threadIdx.x); s < SW * SH; s += int(kTileW * kTileH)) {
        const int sx = s % SW, sy = s / SW;
        const int gx = x0 + sx, gy = y0 + sy;
        if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;   // never read: the tap loop skips it
        const Texel t = load_texel<FIRST>(K, size_t(gy) * K.band_w + uint32_t(gx));
        s_e[s] = t.e;
        s_g[s] = t.g;
    }
    __syncthreads();
    const int tx = int(threadIdx.x % kTileW), ty = int(threadIdx.x / kTileW);
    const int x = x0 + HALO + tx, y = y0 + HALO + ty;
    if (x >= w || y >= h) return;
    const int c = (ty + HALO) * SW + tx + HALO;
    Texel p;
    p.e = s_e[c];
    p.g = s_g[c];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, den = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * STEP;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * STEP;
            if (qx < 0 || qx >= w) continue;
            const int o = c + dy * STEP * SW + dx * STEP;
            Texel q;
            q.e = s_e[o];
            q.g = s_g[o];
            tap(K, p, q, kernel_weight(dy) * kernel_weight(dx), nx, ny, nz, den);
        }
    }
    store_texel<FIRST, LAST>(K, size_t(y) * K.band_w + uint32_t(x), p, nx / den, ny / den, nz / den);
}

namespace rt {

namespace {
template <bool FIRST, bool LAST>
const void* pick_denoise(uint32_t lds_step) {
    switch (lds_step) {
        case 1: return reinterpret_cast<const void*>(rt_denoise_lds_kernel<FIRST, LAST, 1>);
        case 2: return reinterpret_cast<const void*>(rt_denoise_lds_kernel<FIRST, LAST, 2>);
        case 4: return reinterpret_cast<const void*>(rt_denoise_lds_kernel<FIRST, LAST, 4>);
        default: return reinterpret_cast<const void*>(rt_denoise_plain_kernel<FIRST, LAST>);
    }
}
}  // namespace

hipError_t launch_denoise(const DenoiseParams& K, bool first, bool last, uint32_t lds_step, hipStream_t st) {
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (lds_step != 0 && lds_step != 1 && lds_step != 2 && lds_step != 4) return hipErrorInvalidValue;
    const void* fn = first ? (last ? pick_denoise<true, true>(lds_step) : pick_denoise<true, false>(lds_step))
                           : (last ? pick_denoise<false, true>(lds_step) : pick_denoise<false, false>(lds_step));
    void* args[] = {const_cast<DenoiseParams*>(&K)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(fn, grid, dim3(kTileW * kTileH), args, 0, st);
}

}  // namespace rt
