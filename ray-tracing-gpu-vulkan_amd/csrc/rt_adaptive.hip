// rt_adaptive.hip — the kernels of adaptive frames (rt_render_adaptive_device)
// beside the trace kernels: the per-tile noise estimate that builds the next pass's tile list, and
// the resolve with per-tile divisors. Both stream the two fixed-point half-buffers A and B (3 u64
// planes each, TraceParams::fixed layout) once: 48 B per texel, HBM-bound. A third kernel is the
// store of a multi-device adaptive frame on device 0 (rt_multi_render_adaptive): a part's resolved
// band and its count table into the full image.
#include <hip/hip_runtime.h>

#include "rt_adaptive.h"
#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_launchers.h"
#include "rt_sample_map_feedback.h"

using namespace rtd;

namespace {

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace

// One wave per tile of the list, four tiles per block. Lane w owns pixel (w & 7, w >> 3): a row of
// the tile is one 64-byte segment per plane. Lanes outside the band (ragged edge tiles) and waves
// past the list load nothing.
__global__ __launch_bounds__(256) void rt_adaptive_error_kernel(const rt::AdaptiveErrorParams K) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    // the count of the list just consumed is the list after next's: zero it (nothing on the
    // device reads it in this pass, the host passed its value as n_list)
    if (blockIdx.x == 0 && threadIdx.x == 0) K.state->count[K.cur] = 0u;
    if (i >= K.n_list) return;   // wave-uniform
    const uint32_t t = K.list ? K.list[i] : i;
    const uint32_t lx = (t % K.tiles_x) * 8u + (lane & 7u);
    const uint32_t ly = (t / K.tiles_x) * 8u + (lane >> 3);
    const bool in = lx < K.band_w && ly < K.band_h;
    unsigned long long e = 0ull, s = 0ull;
    if (in) {
        const size_t texel = size_t(ly) * K.band_w + lx;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned long long a = K.a[c * K.texels + texel], b = K.b[c * K.texels + texel];
            e += a > b ? a - b : b - a;
            s += a + b;
        }
    }
    e = wave_sum_u64(e);
    s = wave_sum_u64(s);
    const uint32_t m = uint32_t(__popcll(__ballot(in)));
    if (lane != 0u) return;
    const bool conv = rt::adaptive_tile_converged(e, s, K.n_done, m, K.thr_q16);
    K.tile_n[t] = K.n_done;
    if (!conv && K.n_done < K.max_spp) {
        K.next_list[atomicAdd(&K.state->count[K.cur ^ 1u], 1u)] = t;
    } else {
        atomicAdd(&K.state->samples, (unsigned long long)K.n_done * m);
        if (!conv) atomicAdd(&K.state->capped, 1u);
    }
}

// The update of a feedback frame: rt_adaptive_error_kernel's loads and wave reduction over every tile
// of the band, lane 0 applies the rule and writes next[t] (and, for callers with a rule of their
// own, the tile's E and S). No list and no one-address atomic per tile: the counts of raised and
// lowered tiles go through LDS into one atomic per block.
__global__ __launch_bounds__(256) void rt_feedback_update_kernel(const rt::FeedbackParams K) {
    __shared__ unsigned long long s_moved;
    if (threadIdx.x == 0) s_moved = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t < K.n_tiles) {   // wave-uniform
        const uint32_t lx = (t % K.tiles_x) * 8u + (lane & 7u);
        const uint32_t ly = (t / K.tiles_x) * 8u + (lane >> 3);
        const bool in = lx < K.band_w && ly < K.band_h;
        unsigned long long e = 0ull, s = 0ull;
        if (in) {
            const size_t texel = size_t(ly) * K.band_w + lx;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned long long a = K.a[c * K.texels + texel], b = K.b[c * K.texels + texel];
                e += a > b ? a - b : b - a;
                s += a + b;
            }
        }
        e = wave_sum_u64(e);
        s = wave_sum_u64(s);
        const uint32_t m = uint32_t(__popcll(__ballot(in)));
        if (lane == 0u) {
            const uint32_t n = K.tile_n[t];
            const uint32_t next = rt::sample_map_feedback_count(e, s, n, m, K.thr_q16, K.min_spp, K.max_spp);
            K.next[t] = next;
            if (K.tile_error) {
                K.tile_error[2u * t] = e;
                K.tile_error[2u * t + 1u] = s;
            }
            if (next > n) atomicAdd(&s_moved, 1ull);
            if (next < n) atomicAdd(&s_moved, 1ull << 32);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_moved) atomicAdd(K.moved, s_moved);
}

// Per texel: total = A + B, stored as rt_resolve_fixed_kernel stores a launch without
// accumulation, tonemapped with the sample count of the texel's tile; A and B zeroed.
__global__ __launch_bounds__(256) void rt_adaptive_resolve_kernel(unsigned long long* __restrict__ a,
                                                                  unsigned long long* __restrict__ b, uint64_t n,
                                                                  uint32_t band_w, uint32_t tiles_x,
                                                                  const uint32_t* __restrict__ tile_n,
                                                                  float4* __restrict__ accum,
                                                                  uint32_t* __restrict__ out,
                                                                  uint32_t* __restrict__ sample_count) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t y = uint32_t(i) / band_w, x = uint32_t(i) - y * band_w;   // n < 2^32 (band sides < 2^16)
        const uint32_t cnt = tile_n[(y >> 3) * tiles_x + (x >> 3)];
        const unsigned long long q0 = a[i] + b[i], q1 = a[n + i] + b[n + i], q2 = a[2 * n + i] + b[2 * n + i];
        a[i] = 0ull; a[n + i] = 0ull; a[2 * n + i] = 0ull;
        b[i] = 0ull; b[n + i] = 0ull; b[2 * n + i] = 0ull;
        const float s0 = float(double(q0) * 0x1p-24);
        const float s1 = float(double(q1) * 0x1p-24);
        const float s2 = float(double(q2) * 0x1p-24);
        accum[i] = make_float4(s0, s1, s2, 1.0f);
        const float spp = float(cnt);
        out[i] = unorm8(__builtin_sqrtf(s0 / spp)) | (unorm8(__builtin_sqrtf(s1 / spp)) << 8) |
                 (unorm8(__builtin_sqrtf(s2 / spp)) << 16) | (255u << 24);
        if (sample_count) sample_count[i] = cnt;
    }
}

// rt_adaptive_resolve_kernel with the hand-over of the two halves (rt_render_adaptive_halves_device,
// rt_render_sample_map_feedback_halves_device): the same single pass over the
// planes also stores A and B, each resolved as the sum is (an exact product, one rounding), and the
// optional per-texel half count cnt / 2. 156 B per texel instead of 120 B; every float4 is one
// 16-byte store per lane, the plane loads stay 8-byte and wave-contiguous. A sibling and not a
// template of the kernel above: that one's listing stays the parent's (scripts/isa_same.py).
__global__ __launch_bounds__(256) void rt_adaptive_resolve_halves_kernel(
    unsigned long long* __restrict__ a, unsigned long long* __restrict__ b, uint64_t n, uint32_t band_w,
    uint32_t tiles_x, const uint32_t* __restrict__ tile_n, float4* __restrict__ accum, uint32_t* __restrict__ out,
    uint32_t* __restrict__ sample_count, float4* __restrict__ accum_a, float4* __restrict__ accum_b,
    uint32_t* __restrict__ half_count) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t y = uint32_t(i) / band_w, x = uint32_t(i) - y * band_w;   // n < 2^32 (band sides < 2^16)
        const uint32_t cnt = tile_n[(y >> 3) * tiles_x + (x >> 3)];
        const unsigned long long a0 = a[i], a1 = a[n + i], a2 = a[2 * n + i];
        const unsigned long long b0 = b[i], b1 = b[n + i], b2 = b[2 * n + i];
        a[i] = 0ull; a[n + i] = 0ull; a[2 * n + i] = 0ull;
        b[i] = 0ull; b[n + i] = 0ull; b[2 * n + i] = 0ull;
        accum_a[i] = make_float4(float(double(a0) * 0x1p-24), float(double(a1) * 0x1p-24), float(double(a2) * 0x1p-24), 1.0f);
        accum_b[i] = make_float4(float(double(b0) * 0x1p-24), float(double(b1) * 0x1p-24), float(double(b2) * 0x1p-24), 1.0f);
        const float s0 = float(double(a0 + b0) * 0x1p-24);
        const float s1 = float(double(a1 + b1) * 0x1p-24);
        const float s2 = float(double(a2 + b2) * 0x1p-24);
        accum[i] = make_float4(s0, s1, s2, 1.0f);
        const float spp = float(cnt);
        out[i] = unorm8(__builtin_sqrtf(s0 / spp)) | (unorm8(__builtin_sqrtf(s1 / spp)) << 8) |
                 (unorm8(__builtin_sqrtf(s2 / spp)) << 16) | (255u << 24);
        if (sample_count) sample_count[i] = cnt;
        if (half_count) half_count[i] = cnt >> 1;
    }
}

// The store of a multi-device adaptive frame (rt_multi_render_adaptive), on device 0, once per part:
// band row y of `src` (the part's resolved float4 sums, n_rows x width) goes to image row rows[y]
// of the accumulator, the rgba8 image and the optional count map, tonemapped with the count of the
// texel's band tile, in rt_adaptive_resolve_kernel's arithmetic (the same float sum, float(cnt),
// unorm8). One pass over the part instead of a row scatter and a whole-image resolve. The eight
// texels of a tile row share one count word. Map entries >= dst_rows are skipped.
__global__ __launch_bounds__(256) void rt_adaptive_store_tiles_kernel(const float4* __restrict__ src, uint64_t n,
                                                                      uint32_t width, uint32_t tiles_x,
                                                                      const uint32_t* __restrict__ tile_n,
                                                                      const uint32_t* __restrict__ rows,
                                                                      uint32_t dst_rows, float4* __restrict__ accum,
                                                                      uint32_t* __restrict__ out,
                                                                      uint32_t* __restrict__ sample_count) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t y = uint32_t(i) / width, x = uint32_t(i) - y * width;   // n < 2^32 (band sides < 2^16)
        const uint32_t dy = rows[y];
        if (dy >= dst_rows) continue;
        const uint32_t cnt = tile_n[(y >> 3) * tiles_x + (x >> 3)];
        const float4 s = src[i];
        const size_t d = size_t(dy) * width + x;
        accum[d] = s;
        const float spp = float(cnt);
        out[d] = unorm8(__builtin_sqrtf(s.x / spp)) | (unorm8(__builtin_sqrtf(s.y / spp)) << 8) |
                 (unorm8(__builtin_sqrtf(s.z / spp)) << 16) | (255u << 24);
        if (sample_count) sample_count[d] = cnt;
    }
}

namespace rt {

hipError_t launch_adaptive_store_tiles(const float* src, uint32_t n_rows, uint32_t width, const uint32_t* tile_n,
                                       const uint32_t* rows, uint32_t dst_rows, float* accum, uint8_t* out,
                                       uint32_t* sample_count, hipStream_t st) {
    const uint64_t n_texels = uint64_t(n_rows) * width;
    if (n_texels == 0) return hipSuccess;
    const uint64_t need = (n_texels + 255) / 256;
    hipLaunchKernelGGL(rt_adaptive_store_tiles_kernel, dim3(uint32_t(need < 8192 ? need : 8192)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(src), n_texels, width, (width + 7u) / 8u, tile_n, rows, dst_rows,
                       reinterpret_cast<float4*>(accum), reinterpret_cast<uint32_t*>(out), sample_count);
    return hipGetLastError();
}

hipError_t launch_adaptive_init(AdaptiveState* state, hipStream_t st) {
    return hipMemsetAsync(state, 0, sizeof(AdaptiveState), st);
}

hipError_t launch_adaptive_error(const AdaptiveErrorParams& K, hipStream_t st) {
    if (K.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_adaptive_error_kernel, dim3((K.n_list + 3u) / 4u), dim3(256), 0, st, K);
    return hipGetLastError();
}

hipError_t launch_feedback_update(const FeedbackParams& K, hipStream_t st) {
    if (K.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_feedback_update_kernel, dim3((K.n_tiles + 3u) / 4u), dim3(256), 0, st, K);
    return hipGetLastError();
}

hipError_t launch_adaptive_resolve(unsigned long long* a, unsigned long long* b, uint64_t n_texels, uint32_t band_w,
                                   uint32_t tiles_x, const uint32_t* tile_n, float* accum, uint8_t* out,
                                   uint32_t* sample_count, float* accum_a, float* accum_b, uint32_t* half_count,
                                   hipStream_t st) {
    const uint64_t need = (n_texels + 255) / 256;
    const dim3 grid(uint32_t(need < 8192 ? need : 8192));
    if (accum_a)
        hipLaunchKernelGGL(rt_adaptive_resolve_halves_kernel, grid, dim3(256), 0, st, a, b, n_texels, band_w, tiles_x,
                           tile_n, reinterpret_cast<float4*>(accum), reinterpret_cast<uint32_t*>(out), sample_count,
                           reinterpret_cast<float4*>(accum_a), reinterpret_cast<float4*>(accum_b), half_count);
    else
        hipLaunchKernelGGL(rt_adaptive_resolve_kernel, grid, dim3(256), 0, st, a, b, n_texels, band_w, tiles_x, tile_n,
                           reinterpret_cast<float4*>(accum), reinterpret_cast<uint32_t*>(out), sample_count);
    return hipGetLastError();
}

}  // namespace rt
