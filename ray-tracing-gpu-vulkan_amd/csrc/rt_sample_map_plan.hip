// rt_sample_map_plan.hip — the device planner of a sample map (rt_sample_map_set_device_async,
// DESIGN.md §3.1.2): from a device table of per-tile counts, exactly the block table
// rt::sample_map::make_block_plan builds on the host, without the table ever reaching the host. Every
// step is queued on the caller's stream: clamp and key the counts, a stable descending sort of the
// 20-bit keys (equal counts keep the tile order), the choice of the unit from the block totals of
// every candidate, an exclusive scan of the tiles' chunk counts and the expansion into entries. The
// sort and the scan are rocPRIM's; tens of thousands of tiles, not the hot path.
#include <hip/hip_runtime.h>

#include <cstring>   // (rocPRIM's texture iterator calls memset unqualified)

#include <rocprim/rocprim.hpp>

#include "rt_internal.h"
#include "rt_launchers.h"
#include "rt_sample_map_device.h"

using rt::sample_map::DevicePlanParams;
using rt::sample_map::DeviceSummary;
using rt::sample_map::kDeviceUnitSteps;

namespace {

constexpr uint32_t kSums = kDeviceUnitSteps + 2u;   // blocks_at[j], samples, live tiles

// Per tile: the clamped count (the key, and the divisor the resolve reads), the tile index as the
// sort's value, and the tile's share of the summary: its chunks at every candidate unit, its samples
// over its in-band pixels. Sums go through LDS, one global atomic per block and sum.
__global__ __launch_bounds__(256) void rt_map_plan_keys_kernel(const DevicePlanParams K) {
    __shared__ unsigned long long s_sum[kSums];
    __shared__ uint32_t s_max;
    if (threadIdx.x < kSums) s_sum[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < K.n_tiles) {
        const uint32_t raw = K.counts[t];
        uint32_t c = raw < K.count_cap ? raw : K.count_cap;
        if (K.halves) c = (c + 1u) & ~1u;   // (count_cap is even: still <= count_cap)
        const uint32_t key = K.halves ? c / 2u : c;
        K.clamped[t] = c;
        K.keys[t] = key;
        K.vals[t] = t;
        if (c != 0u) {
            const uint32_t tx = t % K.tiles_x, ty = t / K.tiles_x;
            const uint32_t w = min(8u, K.band_w - tx * 8u), h = min(8u, K.band_h - ty * 8u);
            for (uint32_t j = 0; j < kDeviceUnitSteps; j++) {
                const uint32_t unit = rt::sample_map::device_unit_step(K.unit0, j);
                atomicAdd(&s_sum[j], (unsigned long long)((key + unit - 1u) / unit));
            }
            atomicAdd(&s_sum[kDeviceUnitSteps], (unsigned long long)c * w * h);
            atomicAdd(&s_sum[kDeviceUnitSteps + 1u], 1ull);
            atomicMax(&s_max, c);
        }
    }
    __syncthreads();
    if (threadIdx.x < kDeviceUnitSteps) {
        if (s_sum[threadIdx.x]) atomicAdd(&K.summary->blocks_at[threadIdx.x], s_sum[threadIdx.x]);
    } else if (threadIdx.x == kDeviceUnitSteps) {
        if (s_sum[threadIdx.x]) atomicAdd(&K.summary->samples, s_sum[threadIdx.x]);
    } else if (threadIdx.x == kDeviceUnitSteps + 1u) {
        if (s_sum[threadIdx.x]) atomicAdd(&K.summary->live_tiles, uint32_t(s_sum[threadIdx.x]));
        if (s_max) atomicMax(&K.summary->max_count, s_max);
    }
}

// The unit: the first candidate whose table fits the capacity. The last candidate's table is one
// entry per non-zero tile, which the set call has checked against the capacity; should none fit all
// the same, the table is left empty (a frame of it is the 0-sample frame, nothing is overrun).
__global__ void rt_map_plan_pick_kernel(DeviceSummary* __restrict__ s, uint32_t unit0, uint64_t capacity,
                                        uint32_t halves) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t j = 0;
    while (j < kDeviceUnitSteps && s->blocks_at[j] > capacity) j++;
    s->unit_used = rt::sample_map::device_unit_step(unit0, j < kDeviceUnitSteps ? j : kDeviceUnitSteps - 1u);
    const uint32_t n = j < kDeviceUnitSteps ? uint32_t(s->blocks_at[j]) : 0u;
    s->n_blocks = halves ? 2u * n : n;
    s->half_blocks = halves ? n : 0u;
}

// A tile's chunks at the chosen unit, for the scan.
struct ChunksOf {
    const DeviceSummary* s;
    __host__ __device__ uint32_t operator()(uint32_t n) const {
        const uint32_t unit = s->unit_used;
        return (n + unit - 1u) / unit;
    }
};

// One wave per rank of the order, four per block: the k = ceil(n / U) entries of its tile, chunk c =
// samples [c n / k, (c + 1) n / k) in 64-bit arithmetic, from the tile's offset. Nothing is written
// at or past n_blocks (<= the capacity).
__global__ __launch_bounds__(256) void rt_map_plan_expand_kernel(const DevicePlanParams K) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= K.n_tiles) return;
    const uint32_t n = K.keys_sorted[i];
    if (n == 0u) return;
    const uint32_t unit = K.summary->unit_used;
    const uint32_t n_blocks = K.halves ? K.summary->half_blocks : K.summary->n_blocks;
    const uint32_t k = (n + unit - 1u) / unit;
    const uint32_t off = K.offsets[i], tile = K.order[i];
    rt::BlockEntry* out = static_cast<rt::BlockEntry*>(K.blocks);
    for (uint32_t c = lane; c < k; c += 64u) {
        if (uint64_t(off) + c >= n_blocks) break;
        const uint32_t s0 = uint32_t(uint64_t(c) * n / k), s1 = uint32_t((uint64_t(c) + 1u) * n / k);
        out[off + c] = rt::BlockEntry{tile, s0, s1, 0u};
        if (K.halves) {   // the B half: behind the A half, and once more at its fixed place
            const rt::BlockEntry b{tile, s0 + n, s1 + n, 0u};
            out[n_blocks + off + c] = b;
            out[2u * K.capacity + off + c] = b;
        }
    }
}

}  // namespace

namespace rt {

// Bytes of `temp` for a map of n_tiles tiles: host only, independent of the data.
hipError_t device_plan_temp_bytes(uint32_t n_tiles, size_t* bytes) {
    size_t sort_bytes = 0, scan_bytes = 0;
    uint32_t* p = nullptr;
    if (hipError_t e = rocprim::radix_sort_pairs_desc(nullptr, sort_bytes, p, p, p, p, n_tiles, 0u, 20u); e != hipSuccess)
        return e;
    auto in = rocprim::make_transform_iterator(p, ChunksOf{nullptr});
    if (hipError_t e = rocprim::exclusive_scan(nullptr, scan_bytes, in, p, 0u, n_tiles, rocprim::plus<uint32_t>());
        e != hipSuccess)
        return e;
    *bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    return hipSuccess;
}

hipError_t launch_device_plan(const DevicePlanParams& K, hipStream_t st) {
    if (hipError_t e = hipMemsetAsync(K.summary, 0, sizeof(DeviceSummary), st); e != hipSuccess) return e;
    hipLaunchKernelGGL(rt_map_plan_keys_kernel, dim3((K.n_tiles + 255u) / 256u), dim3(256), 0, st, K);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    size_t bytes = size_t(K.temp_bytes);
    // counts <= 2^19: 20 key bits; the sort is stable, so equal counts stay in tile order
    if (hipError_t e = rocprim::radix_sort_pairs_desc(K.temp, bytes, K.keys, K.keys_sorted, K.vals, K.order, K.n_tiles,
                                                      0u, 20u, st);
        e != hipSuccess)
        return e;
    hipLaunchKernelGGL(rt_map_plan_pick_kernel, dim3(1), dim3(64), 0, st, K.summary, K.unit0, K.capacity, K.halves);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    bytes = size_t(K.temp_bytes);
    auto in = rocprim::make_transform_iterator(K.keys_sorted, ChunksOf{K.summary});
    if (hipError_t e = rocprim::exclusive_scan(K.temp, bytes, in, K.offsets, 0u, K.n_tiles, rocprim::plus<uint32_t>(), st);
        e != hipSuccess)
        return e;
    hipLaunchKernelGGL(rt_map_plan_expand_kernel, dim3((K.n_tiles + 3u) / 4u), dim3(256), 0, st, K);
    return hipGetLastError();
}

}  // namespace rt
