// rt_frame_kernels.hip — the kernels around a trace launch that trace nothing: the per-launch
// preparation, the size record of a device-planned block table, the HASH-mode resolve
// (shader.rgen:53-66 for the chunked frame), the band-row scatter and gather of multi-device frames,
// and the tonemap of a summed accumulator (shader.rgen:65-66); with their launchers.
#include <hip/hip_runtime.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_launchers.h"

using namespace rtd;

namespace {

// The big-sphere table of a launch (TraceParams::big_tab): records {cx, cy, cz, r} of the n_big
// spheres, padded to a multiple of 4 by repeating the last (a duplicate never changes (best, bi)),
// then their ids. One wave, before the trace kernel on the same stream.
// Per-launch preparation in one kernel instead of five stream operations: block 0
// zeroes the counters, starts the first-time stamps at the maximum (atomicMin), sets the work
// counter past the blocks the waves take by wave id, and fills the big-sphere table; every block
// zeroes its share of the tile-cost table this launch records into.
__global__ __launch_bounds__(256) void rt_launch_prep_kernel(rt::Counters* __restrict__ counters, uint32_t work_head,
                                                             const rt::GeomRec* __restrict__ geom,
                                                             const float* __restrict__ radius,
                                                             const uint32_t* __restrict__ big_ids, uint32_t n_big,
                                                             float4* __restrict__ tab, uint32_t* __restrict__ cost,
                                                             uint32_t n_cost) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_cost; i += gridDim.x * 256u) cost[i] = 0u;
    if (blockIdx.x != 0) return;
    static_assert(sizeof(rt::Counters) % 8 == 0, "counters are zeroed as u64 words");
    unsigned long long* w = reinterpret_cast<unsigned long long*>(counters);
    for (uint32_t i = threadIdx.x; i < sizeof(rt::Counters) / 8u; i += 256u) w[i] = 0ull;
    const uint32_t nb4 = (n_big + 3u) & ~3u;
    if (threadIdx.x < nb4 && n_big != 0u) {
        const uint32_t id = big_ids[min(threadIdx.x, n_big - 1u)];
        const rt::GeomRec g = geom[id];
        tab[threadIdx.x] = make_float4(g.cx, g.cy, g.cz, radius[id]);
        reinterpret_cast<uint32_t*>(tab + rt::kBigMax)[threadIdx.x] = id;
    }
    if (n_big == 0u && threadIdx.x < 4u) {   // four inert records (setup_ray tests the first four
        // unconditionally): centre (1e19, 1e19, 1e19), radius 0: c = |oc|^2 >= 0 and D <= 0 by
        // Cauchy-Schwarz, and any rounding-made candidate reports t ~ 1e19 > tMax
        tab[threadIdx.x] = make_float4(1e19f, 1e19f, 1e19f, 0.0f);
        reinterpret_cast<uint32_t*>(tab + rt::kBigMax)[threadIdx.x] = 0xffffffffu;
    }
    __syncthreads();   // the words below were zeroed by other threads of the block
    if (threadIdx.x == 0) {
        counters->t_first = ~0ull;
        counters->t_dry = ~0ull;
        counters->work_head = work_head;
    }
}

// The sizes of a table launch whose table was planned on the device (rt_sample_map_plan.hip): from
// the block count in device memory, the record the trace kernel reads at entry (TraceParams::
// tab_size) and the work counter past the first blocks, by the host plan's own rule (rt_hand_out.h).
// One thread, after rt_launch_prep_kernel on the launch's stream. n_blocks <= 2^23 (the planner's
// capacity, twice in halves mode), so 64 n_blocks fits 32 bits.
__global__ void rt_tab_size_kernel(const uint32_t* __restrict__ n_blocks, uint32_t reserve, uint32_t grid_waves,
                                   rt::TabSize* __restrict__ rec, rt::Counters* __restrict__ counters) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t n_units = *n_blocks * 64u;
    const rt::HandOut h = rt::hand_out(n_units, reserve, grid_waves);
    *rec = rt::TabSize{n_units, h.n_block_units, h.first_blocks, 0u};
    counters->work_head = 64u * h.first_blocks;
}

// HASH-mode resolve (shader.rgen:53-66 for the chunked frame): per texel, the fixed-point sum of
// this launch's samples plus the incoming float accumulator (accumulate = 1), rounded once to
// float, stored with alpha 1, tonemapped to rgba8; the fixed-point planes are zeroed for the next
// launch. HBM-bound: 24 B read + 24 B zeroed + 20 B stored per texel (+16 B read when accumulating).
__global__ __launch_bounds__(256) void rt_resolve_fixed_kernel(unsigned long long* __restrict__ fixed, uint64_t n,
                                                               uint32_t accumulate, float spp,
                                                               float4* __restrict__ accum,
                                                               uint32_t* __restrict__ out) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const unsigned long long q0 = fixed[i], q1 = fixed[n + i], q2 = fixed[2 * n + i];
        fixed[i] = 0ull;
        fixed[n + i] = 0ull;
        fixed[2 * n + i] = 0ull;
        const float4 a = accumulate ? accum[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float s0 = float(double(a.x) + double(q0) * 0x1p-24);
        const float s1 = float(double(a.y) + double(q1) * 0x1p-24);
        const float s2 = float(double(a.z) + double(q2) * 0x1p-24);
        accum[i] = make_float4(s0, s1, s2, 1.0f);
        out[i] = unorm8(__builtin_sqrtf(s0 / spp)) | (unorm8(__builtin_sqrtf(s1 / spp)) << 8) |
                 (unorm8(__builtin_sqrtf(s2 / spp)) << 16) | (255u << 24);
    }
}

// Band rows -> full image rows (the reorder after the multi-GPU gather).
// Rows mapping at or beyond dst_rows are skipped (the host validates the map; this keeps a bad
// map from writing out of bounds).
__global__ __launch_bounds__(256) void rt_scatter_rows_kernel(const float4* __restrict__ src_acc,
                                                              const uint32_t* __restrict__ src_px,
                                                              const uint32_t* __restrict__ rows,
                                                              uint32_t n_rows, uint32_t width, uint32_t dst_rows,
                                                              float4* __restrict__ dst_acc,
                                                              uint32_t* __restrict__ dst_px) {
    const uint32_t r = blockIdx.y;
    if (r >= n_rows) return;
    const uint32_t dr = rows[r];
    if (dr >= dst_rows) return;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < width; x += gridDim.x * blockDim.x) {
        if (dst_acc) dst_acc[size_t(dr) * width + x] = src_acc[size_t(r) * width + x];
        if (dst_px) dst_px[size_t(dr) * width + x] = src_px[size_t(r) * width + x];
    }
}

// Full image rows -> band rows (the inverse of rt_scatter_rows_kernel): the running sums an
// accumulating multi-GPU frame hands each device before it renders (rt_multi.cpp). Rows mapping at
// or beyond src_rows leave their band row untouched.
__global__ __launch_bounds__(256) void rt_gather_rows_kernel(const float4* __restrict__ src_acc,
                                                             const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                             uint32_t width, uint32_t src_rows,
                                                             float4* __restrict__ dst_acc) {
    const uint32_t r = blockIdx.y;
    if (r >= n_rows) return;
    const uint32_t sr = rows[r];
    if (sr >= src_rows) return;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < width; x += gridDim.x * blockDim.x)
        dst_acc[size_t(r) * width + x] = src_acc[size_t(sr) * width + x];
}

// Tonemap of a summed accumulator, exactly the trace kernel's pixel store (shader.rgen:65-66).
__global__ __launch_bounds__(256) void rt_tonemap_kernel(const float4* __restrict__ acc, uint64_t n, float spp,
                                                         uint32_t* __restrict__ out) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        const float4 s = acc[i];
        out[i] = unorm8(__builtin_sqrtf(s.x / spp)) | (unorm8(__builtin_sqrtf(s.y / spp)) << 8) |
                 (unorm8(__builtin_sqrtf(s.z / spp)) << 16) | (255u << 24);
    }
}

}  // namespace

// ---- host-callable launchers (rt_launchers.h) -----------------------------------------------
namespace rt {

static uint32_t stream_blocks(uint64_t n) {
    const uint64_t need = (n + 255) / 256;
    return uint32_t(need < 8192 ? need : 8192);
}

hipError_t launch_prep(const TraceParams& P, uint32_t work_head, float* tab, uint32_t n_cost, hipStream_t st) {
    const uint32_t blocks = n_cost > 4096u ? min(64u, (n_cost + 4095u) / 4096u) : 1u;
    hipLaunchKernelGGL(rt_launch_prep_kernel, dim3(blocks), dim3(256), 0, st, P.counters, work_head, P.geom, P.radius,
                       P.big_ids, P.n_big, reinterpret_cast<float4*>(tab), P.tile_cost, n_cost);
    return hipGetLastError();
}

hipError_t launch_tab_size(const uint32_t* n_blocks, uint64_t reserve, uint64_t grid_waves, TabSize* rec,
                           Counters* counters, hipStream_t st) {
    const uint32_t cap = 0xffffffffu;   // (a reserve or grid beyond 32 bits acts as one of 2^32 - 1: n_units < 2^31)
    hipLaunchKernelGGL(rt_tab_size_kernel, dim3(1), dim3(64), 0, st, n_blocks, uint32_t(reserve < cap ? reserve : cap),
                       uint32_t(grid_waves < cap ? grid_waves : cap), rec, counters);
    return hipGetLastError();
}

hipError_t launch_resolve_fixed(unsigned long long* fixed, uint64_t n_texels, uint32_t accumulate, uint32_t spp,
                                float* accum, uint8_t* out, hipStream_t st) {
    if (n_texels == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_resolve_fixed_kernel, dim3(stream_blocks(n_texels)), dim3(256), 0, st, fixed, n_texels,
                       accumulate, float(spp), reinterpret_cast<float4*>(accum), reinterpret_cast<uint32_t*>(out));
    return hipGetLastError();
}

hipError_t launch_scatter_rows(const float* src_acc, const uint8_t* src_px, const uint32_t* rows,
                               uint32_t n_rows, uint32_t width, uint32_t dst_rows, float* dst_acc, uint8_t* dst_px,
                               hipStream_t st) {
    if (n_rows == 0 || width == 0) return hipSuccess;
    dim3 g((width + 255) / 256, n_rows), b(256);
    hipLaunchKernelGGL(rt_scatter_rows_kernel, g, b, 0, st,
                       reinterpret_cast<const float4*>(src_acc), reinterpret_cast<const uint32_t*>(src_px),
                       rows, n_rows, width, dst_rows, reinterpret_cast<float4*>(dst_acc),
                       reinterpret_cast<uint32_t*>(dst_px));
    return hipGetLastError();
}

hipError_t launch_gather_rows(const float* src_acc, const uint32_t* rows, uint32_t n_rows, uint32_t width,
                              uint32_t src_rows, float* dst_acc, hipStream_t st) {
    if (n_rows == 0 || width == 0) return hipSuccess;
    dim3 g((width + 255) / 256, n_rows), b(256);
    hipLaunchKernelGGL(rt_gather_rows_kernel, g, b, 0, st, reinterpret_cast<const float4*>(src_acc), rows, n_rows,
                       width, src_rows, reinterpret_cast<float4*>(dst_acc));
    return hipGetLastError();
}

hipError_t launch_tonemap(const float* accum, uint64_t n_texels, uint32_t spp, uint8_t* out, hipStream_t st) {
    if (n_texels == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_tonemap_kernel, dim3(stream_blocks(n_texels)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(accum), n_texels, float(spp), reinterpret_cast<uint32_t*>(out));
    return hipGetLastError();
}

}  // namespace rt
