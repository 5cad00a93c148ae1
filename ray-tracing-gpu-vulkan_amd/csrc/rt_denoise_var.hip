// rt_denoise_var.hip — the kernels of rt_denoise_variance_device (include/rt_mi355x.h, DESIGN.md
// §3.1.3): rt_denoise.hip's a-trous filter with a colour weight scaled by a per-texel variance that
// is estimated from two half-buffers, smoothed by feature-only prefilter passes and carried through
// the iterations. One kernel per pass or iteration, one thread per texel, blocks of kTileW x kTileH
// texels, as there. The first launch computes its inputs from the caller's buffers (the prologue:
// e_0, v_0, nrm, z) and stores the guide plane; the last iteration multiplies the albedo back and
// tonemaps (the epilogue). Every operation is one correctly rounded binary32 + - x / in the order
// the contract writes it (the library is built with -ffp-contract=off, never -ffast-math).
//
// A texel's filter state is two float4: E = (e.rgb, v) and G = (nrm.xyz, z); the variance rides in
// the slot the plain filter leaves 0, so the context's planes serve both filters. Launches of small
// step stage their tile and its halo of 2 step texels in LDS once (an iteration E and G, 32 B per
// texel; a prefilter pass G and v, 20 B); the others read their taps from global memory. Both forms
// run the same tap loop on the same values, so they give the same bits.
#include <hip/hip_runtime.h>

#include "rt_denoise_host.h"
#include "rt_denoise_var.h"
#include "rt_device_math.h"

using namespace rtd;

namespace {

constexpr uint32_t kTileW = rt::denoise::kTileW, kTileH = rt::denoise::kTileH;
constexpr float kVarFloor = 0x1p-20f;

struct Texel {
    float4 e, g;   // (e.rgb, v), (nrm.xyz, z)
};

// The prologue for texel i: pa, pb = A.rgb / h, B.rgb / h (0 for h = 0), a = feat0.rgb / F + 2^-6,
// e_0 = ((pa + pb) * 0.5) / a, d = (pa - pb) / a, v_0 = 0.25 (d . d), nrm = feat1.xyz / F,
// z = feat1.w / F.
__device__ __forceinline__ Texel prologue(const rt::DenoiseVarParams& K, size_t i) {
    const float4 A = reinterpret_cast<const float4*>(K.accum_a)[i];
    const float4 B = reinterpret_cast<const float4*>(K.accum_b)[i];
    const float4 f0 = reinterpret_cast<const float4*>(K.feat0)[i];
    const float4 f1 = reinterpret_cast<const float4*>(K.feat1)[i];
    const uint32_t h = K.half_count ? K.half_count[i] : K.half_spp;
    const float hf = float(h), F = K.feature_samples;
    const float pax = h ? A.x / hf : 0.0f, pay = h ? A.y / hf : 0.0f, paz = h ? A.z / hf : 0.0f;
    const float pbx = h ? B.x / hf : 0.0f, pby = h ? B.y / hf : 0.0f, pbz = h ? B.z / hf : 0.0f;
    const float ax = f0.x / F + 0x1p-6f, ay = f0.y / F + 0x1p-6f, az = f0.z / F + 0x1p-6f;
    const float dx = (pax - pbx) / ax, dy = (pay - pby) / ay, dz = (paz - pbz) / az;
    Texel t;
    t.e = make_float4(((pax + pbx) * 0.5f) / ax, ((pay + pby) * 0.5f) / ay, ((paz + pbz) * 0.5f) / az,
                      0.25f * ((dx * dx + dy * dy) + dz * dz));
    t.g = make_float4(f1.x / F, f1.y / F, f1.z / F, f1.w / F);
    return t;
}

template <bool FIRST>
__device__ __forceinline__ Texel load_texel(const rt::DenoiseVarParams& K, size_t i) {
    if constexpr (FIRST) {
        return prologue(K, i);
    } else {
        Texel t;
        t.e = reinterpret_cast<const float4*>(K.src)[i];
        t.g = reinterpret_cast<const float4*>(K.guide)[i];
        return t;
    }
}

// What a prefilter tap reads of texel i: G and v alone.
template <bool FIRST>
__device__ __forceinline__ void load_gv(const rt::DenoiseVarParams& K, size_t i, float4& g, float& v) {
    if constexpr (FIRST) {
        const Texel t = prologue(K, i);
        g = t.g;
        v = t.e.w;
    } else {
        g = reinterpret_cast<const float4*>(K.guide)[i];
        v = K.src[4u * i + 3u];
    }
}

// f(p, q) = (1 + k_normal dn2) (1 + k_depth (dz dz))
__device__ __forceinline__ float feature_stop(const rt::DenoiseVarParams& K, const float4& pg, const float4& qg) {
    const float dnx = pg.x - qg.x, dny = pg.y - qg.y, dnz = pg.z - qg.z;
    const float dn2 = (dnx * dnx + dny * dny) + dnz * dnz;
    const float dz = (pg.w - qg.w) / (pg.w + 1.0f);
    return (1.0f + K.k_normal * dn2) * (1.0f + K.k_depth * (dz * dz));
}

// One prefilter tap of weight kk = K[|dy|] K[|dx|] at texel q, seen from p.
__device__ __forceinline__ void tap_prefilter(const rt::DenoiseVarParams& K, const float4& pg, const float4& qg, float qv,
                                              float kk, float& nv, float& den) {
    const float f = feature_stop(K, pg, qg);
    const float w = kk / (f * f);
    nv += w * qv;
    den += w;
}

struct Sums {
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, den = 0.0f, nv = 0.0f;
};

// One iteration tap; vp = v_i(p) + 2^-20.
__device__ __forceinline__ void tap(const rt::DenoiseVarParams& K, const Texel& p, float vp, const Texel& q, float kk,
                                    Sums& s) {
    const float f = feature_stop(K, p.g, q.g);
    const float dex = p.e.x - q.e.x, dey = p.e.y - q.e.y, dez = p.e.z - q.e.z;
    const float de2 = (dex * dex + dey * dey) + dez * dez;
    const float x = f * (1.0f + K.k_color * (de2 / vp));
    const float w = kk / (x * x);
    s.nx += w * q.e.x;
    s.ny += w * q.e.y;
    s.nz += w * q.e.z;
    s.den += w;
    s.nv += (w * w) * q.e.w;
}

__device__ __forceinline__ float kernel_weight(int d) {   // the B3 spline {1, 4, 6, 4, 1} / 16
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// E' = (e', v') stored, or with LAST the epilogue: mean = e' a, (mean, 1) and its rgba8.
template <bool FIRST, bool LAST>
__device__ __forceinline__ void store_texel(const rt::DenoiseVarParams& K, size_t i, const float4& g, float ex, float ey,
                                            float ez, float v) {
    if constexpr (FIRST && !LAST) reinterpret_cast<float4*>(K.guide_out)[i] = g;
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
        reinterpret_cast<float4*>(K.dst)[i] = make_float4(ex, ey, ez, v);
    }
}

}  // namespace

// ---- iterations -------------------------------------------------------------------------------

// Taps from global memory (the large steps; any step in the forced form of the tests).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_var_plain_kernel(const rt::DenoiseVarParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const Texel p = load_texel<FIRST>(K, i);
    const float vp = p.e.w + kVarFloor;
    Sums s;
    const int step = int(K.step), w = int(K.band_w), h = int(K.band_h);
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = int(y) + dy * step;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = int(x) + dx * step;
            if (qx < 0 || qx >= w) continue;
            const Texel q = load_texel<FIRST>(K, size_t(qy) * K.band_w + uint32_t(qx));
            tap(K, p, vp, q, kernel_weight(dy) * kernel_weight(dx), s);
        }
    }
    store_texel<FIRST, LAST>(K, i, p.g, s.nx / s.den, s.ny / s.den, s.nz / s.den, s.nv / (s.den * s.den));
}

// Taps from LDS: the block stages the texels [x0 - 2 STEP, x0 + kTileW + 2 STEP) x [y0 - 2 STEP,
// y0 + kTileH + 2 STEP) that lie in the band (with FIRST, their prologue once per texel instead of
// once per tap), then every thread reads its 25 taps there.
template <bool FIRST, bool LAST, int STEP>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_var_lds_kernel(const rt::DenoiseVarParams K) {
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
    const float vp = p.e.w + kVarFloor;
    Sums s;
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
            tap(K, p, vp, q, kernel_weight(dy) * kernel_weight(dx), s);
        }
    }
    store_texel<FIRST, LAST>(K, size_t(y) * K.band_w + uint32_t(x), p.g, s.nx / s.den, s.ny / s.den, s.nz / s.den,
                             s.nv / (s.den * s.den));
}

// ---- prefilter passes: v alone, e carried over ---------------------------------------------------

template <bool FIRST>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_var_pre_plain_kernel(const rt::DenoiseVarParams K) {
    const uint32_t x = blockIdx.x * kTileW + (threadIdx.x % kTileW);
    const uint32_t y = blockIdx.y * kTileH + (threadIdx.x / kTileW);
    if (x >= K.band_w || y >= K.band_h) return;
    const size_t i = size_t(y) * K.band_w + x;
    const Texel p = load_texel<FIRST>(K, i);
    float nv = 0.0f, den = 0.0f;
    const int step = int(K.step), w = int(K.band_w), h = int(K.band_h);
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = int(y) + dy * step;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = int(x) + dx * step;
            if (qx < 0 || qx >= w) continue;
            float4 qg;
            float qv;
            load_gv<FIRST>(K, size_t(qy) * K.band_w + uint32_t(qx), qg, qv);
            tap_prefilter(K, p.g, qg, qv, kernel_weight(dy) * kernel_weight(dx), nv, den);
        }
    }
    store_texel<FIRST, false>(K, i, p.g, p.e.x, p.e.y, p.e.z, nv / den);
}

template <bool FIRST, int STEP>
__global__ __launch_bounds__(kTileW* kTileH) void rt_denoise_var_pre_lds_kernel(const rt::DenoiseVarParams K) {
    constexpr int HALO = 2 * STEP, SW = int(kTileW) + 2 * HALO, SH = int(kTileH) + 2 * HALO;
    __shared__ float4 s_g[SW * SH];
    __shared__ float s_v[SW * SH];
    const int x0 = int(blockIdx.x * kTileW) - HALO, y0 = int(blockIdx.y * kTileH) - HALO;
    const int w = int(K.band_w), h = int(K.band_h);
    for (int s = int(threadIdx.x); s < SW * SH; s += int(kTileW * kTileH)) {
        const int sx = s % SW, sy = s / SW;
        const int gx = x0 + sx, gy = y0 + sy;
        if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;   // never read: the tap loop skips it
        float4 g;
        float v;
        load_gv<FIRST>(K, size_t(gy) * K.band_w + uint32_t(gx), g, v);
        s_g[s] = g;
        s_v[s] = v;
    }
    __syncthreads();
    const int tx = int(threadIdx.x % kTileW), ty = int(threadIdx.x / kTileW);
    const int x = x0 + HALO + tx, y = y0 + HALO + ty;
    if (x >= w || y >= h) return;
    const int c = (ty + HALO) * SW + tx + HALO;
    const size_t i = size_t(y) * K.band_w + uint32_t(x);
    const float4 pg = s_g[c];
    float nv = 0.0f, den = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * STEP;
        if (qy < 0 || qy >= h) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * STEP;
            if (qx < 0 || qx >= w) continue;
            const int o = c + dy * STEP * SW + dx * STEP;
            tap_prefilter(K, pg, s_g[o], s_v[o], kernel_weight(dy) * kernel_weight(dx), nv, den);
        }
    }
    // the texel's own e: the one value of the pass that is not staged
    const Texel p = load_texel<FIRST>(K, i);
    store_texel<FIRST, false>(K, i, pg, p.e.x, p.e.y, p.e.z, nv / den);
}

namespace rt {

namespace {
template <bool FIRST, bool LAST>
const void* pick_iteration(uint32_t lds_step) {
    switch (lds_step) {
        case 1: return reinterpret_cast<const void*>(rt_denoise_var_lds_kernel<FIRST, LAST, 1>);
        case 2: return reinterpret_cast<const void*>(rt_denoise_var_lds_kernel<FIRST, LAST, 2>);
        case 4: return reinterpret_cast<const void*>(rt_denoise_var_lds_kernel<FIRST, LAST, 4>);
        default: return reinterpret_cast<const void*>(rt_denoise_var_plain_kernel<FIRST, LAST>);
    }
}
template <bool FIRST>
const void* pick_prefilter(uint32_t lds_step) {
    switch (lds_step) {
        case 1: return reinterpret_cast<const void*>(rt_denoise_var_pre_lds_kernel<FIRST, 1>);
        case 2: return reinterpret_cast<const void*>(rt_denoise_var_pre_lds_kernel<FIRST, 2>);
        case 4: return reinterpret_cast<const void*>(rt_denoise_var_pre_lds_kernel<FIRST, 4>);
        default: return reinterpret_cast<const void*>(rt_denoise_var_pre_plain_kernel<FIRST>);
    }
}
}  // namespace

hipError_t launch_denoise_var(const DenoiseVarParams& K, bool prefilter, bool first, bool last, uint32_t lds_step,
                              hipStream_t st) {
    if (K.band_w == 0 || K.band_h == 0) return hipSuccess;
    if (lds_step != 0 && lds_step != 1 && lds_step != 2 && lds_step != 4) return hipErrorInvalidValue;
    if (prefilter && last) return hipErrorInvalidValue;   // the epilogue belongs to an iteration
    const void* fn;
    if (prefilter) fn = first ? pick_prefilter<true>(lds_step) : pick_prefilter<false>(lds_step);
    else
        fn = first ? (last ? pick_iteration<true, true>(lds_step) : pick_iteration<true, false>(lds_step))
                   : (last ? pick_iteration<false, true>(lds_step) : pick_iteration<false, false>(lds_step));
    void* args[] = {const_cast<DenoiseVarParams*>(&K)};
    const dim3 grid((K.band_w + kTileW - 1u) / kTileW, (K.band_h + kTileH - 1u) / kTileH);
    return hipLaunchKernel(fn, grid, dim3(kTileW * kTileH), args, 0, st);
}

}  // namespace rt
