// rt_trace_units.h — a lane's work unit and how the trace kernels hand units out (device only):
//   shaders/shader.rgen:40      the pixel seed, TEA(TEA(x, y), number) (tile_pixel_seed)
//   shaders/shader.rgen:53-55   the incoming accumulator and the dvec3 sum (begin_unit, Path)
//   shaders/shader.rgen:61-66   the finished pixel's store and rgba8 resolve (store_pixel)
// and, with no reference counterpart, the per-lane path state, the counter-based stream's sample
// seed and 8.24 fixed-point sums, the row map, the block hand-out (uniform and table form), refill,
// tail stealing, the first block of a wave and the tile-cost record.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"
#include "rt_trace_prims.h"

using namespace rtd;

namespace {

enum : uint32_t { ST_NEED_UNIT = 0, ST_NEED_SAMPLE = 1, ST_TRACING = 2, ST_RETIRED = 3 };

// One lane's work unit: samples [s, s_end) of pixel px. STREAM sums in double (the dvec3 of
// shader.rgen:55); HASH sums 8.24 fixed point (q) over at most kFixedFlush samples, then adds the
// partial to the pixel's 64-bit sum in HBM.
struct Path {
    uint32_t px;           // lx | ly << 16 (band-local launch id)
    uint32_t pixel_seed;   // TEA(TEA(x, y), number)
    uint32_t seed;         // LCG state (random.glsl)
    uint32_t s, s_end;     // next sample of the unit, end of the unit's samples
    uint32_t depth;        // segments traced in this sample
    uint32_t segs;         // segments traced for this unit (tile cost for the hand-out order)
    V3 thr;                // reflectedColor (shader.rgen:71)
    double sx, sy, sz;     // STREAM: dvec3 sum
    uint32_t qx, qy, qz;   // HASH: fixed-point partial sum since the last flush
};
// FEATURES: the unit's binary32 sums, in sample order. A type of its own, so that the other modes'
// Path, and with it their code, is what it was: the kernels declare PathOf<MODE>, the functions
// take a Path&, and the FEATURES branches (if constexpr) see the whole object (feat_path).
struct FeatPath : Path {
    float far, fag, fab, fah;   // albedo.rgb, hit
    float fnx, fny, fnz, fdz;   // n.xyz, depth
};
template <int MODE> struct PathType { typedef Path type; };
template <> struct PathType<rt::MODE_FEATURES> { typedef FeatPath type; };
template <int MODE> using PathOf = typename PathType<MODE>::type;
__device__ __forceinline__ FeatPath& feat_path(Path& ps) { return static_cast<FeatPath&>(ps); }
// Global load of a rarely taken branch, waited for at once. vmcnt counts loads and stores alike
// (gfx9): a load left pending across a branch makes the compiler wait vmcnt(0) at the loop head
// (the register is reused there), which then also waits for the pixel stores still in flight —
// about 10 us per finished pixel. Waiting here, inside the branch, keeps the head
// free of it.
typedef const volatile __attribute__((address_space(1))) uint32_t* GlobalVU32;
typedef const volatile __attribute__((address_space(1))) f4v* GlobalVF4;
__device__ __forceinline__ uint32_t load_now(const uint32_t* p) {
    const uint32_t v = *(GlobalVU32)p;
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt/lgkmcnt untouched
    return v;
}
__device__ __forceinline__ float4 load_now4(const float4* p) {
    const f4v v = *(GlobalVF4)p;
    __builtin_amdgcn_s_waitcnt(0x0F70);
    return make_float4(v.x, v.y, v.z, v.w);
}
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(1))) u4v* GlobalVU4;
__device__ __forceinline__ rt::BlockEntry load_now_block(const rt::BlockEntry* p) {
    const u4v v = *(GlobalVU4)p;
    __builtin_amdgcn_s_waitcnt(0x0F70);
    return rt::BlockEntry{v.x, v.y, v.z, v.w};
}

// RT_RNG_SAMPLE_HASH: LCG start of sample s of a pixel. One multiply-add
// spreads consecutive sample indices (golden ratio), then the "lowbias32" integer finaliser
// (two multiplies, three xor-shifts) scrambles: ~8 VALU per sample instead of a 16-round TEA.
__device__ __forceinline__ uint32_t sample_seed_hash(uint32_t pixel_seed, uint32_t s) {
    uint32_t x = pixel_seed + 0x9E3779B9u * s;
    x ^= x >> 16;
    x *= 0x21F0AAADu;
    x ^= x >> 15;
    x *= 0x735A2D97u;
    x ^= x >> 15;
    return x;
}

// RT_RNG_SAMPLE_HASH accumulation: a colour channel in [0, 1] as 8.24 fixed point, truncated
// (rt_internal.h kFixedFracBits). Integer sums are associative, so the order in which chunks and
// partial sums of a pixel land does not change a bit. The clamp only defines NaN (-> 0); colours
// lie in [0, 1].
__device__ __forceinline__ uint32_t sample_fixed(float c) {
    const float v = fminf(fmaxf(c, 0.0f), 1.0f) * 0x1p24f;
    return uint32_t(v);
}

// Adds fixed-point sums to a pixel's 64-bit sums in HBM (fire-and-forget relaxed atomics);
// rt_resolve_fixed_kernel stores the pixel.
__device__ __forceinline__ void add_fixed(const rt::TraceParams& P, const Path& ps, unsigned long long x,
                                          unsigned long long y, unsigned long long z) {
    const uint32_t lx = ps.px & 0xffffu, ly = ps.px >> 16;
    const size_t n = size_t(P.band_w) * P.band_h, texel = size_t(ly) * P.band_w + lx;
    __hip_atomic_fetch_add(P.fixed + texel, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(P.fixed + n + texel, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(P.fixed + 2 * n + texel, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Per-lane 64-bit unit sums in LDS (LSUM kernels: the grid kernels, whose LDS has room for them,
// 24 B per thread): the 32-bit lane partial, which must be emptied every kFixedFlush samples, is
// added here, and the unit's sum goes to HBM once when the unit ends, instead of three
// device-scope atomics per lane every kFixedFlush samples (config 3: ~486 M atomics, 16 GB of
// memory-side write requests per frame). Lane-private slots: no contention.
__shared__ unsigned long long s_lane_sum[3 * RT_TRACE_BLOCK];
// A thread's slot from the wave's first thread (wave-uniform: an SGPR) and the lane id (mbcnt),
// so no thread-id VGPR stays live across the segment loop for it.
__device__ __forceinline__ unsigned long long* lane_sum_slot() {
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    return s_lane_sum + wave0 + __lane_id();
}
static_assert(sizeof(s_lane_sum) == rt::kLaneSumLdsBytes, "rt_internal.h");

// Empties a lane's 32-bit partial sums (every kFixedFlush samples and at the unit's end).
template <bool LSUM>
__device__ __forceinline__ void flush_fixed(const rt::TraceParams& P, Path& ps) {
    if (LSUM) {
        unsigned long long* s = lane_sum_slot();   // ds_add_u64 without return: no read back
        __hip_atomic_fetch_add(s, (unsigned long long)ps.qx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(s + RT_TRACE_BLOCK, (unsigned long long)ps.qy, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(s + 2 * RT_TRACE_BLOCK, (unsigned long long)ps.qz, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WAVEFRONT);
    } else {
        add_fixed(P, ps, ps.qx, ps.qy, ps.qz);
    }
    ps.qx = ps.qy = ps.qz = 0u;
}

// Global row of band row ly: the row map (rows), staged in LDS by the walk kernels when it fits
// their LDS plan (an lgkmcnt wait instead of a global load whose vmcnt(0) wait also drains the
// wave's stores and atomics; N > 1 strips: one per sample start), else loaded
// from global memory; without a map, off_y + ly.
extern __shared__ float4 rt_dyn_lds[];   // the dynamic LDS of the launch (the kernels' `lds`)
__device__ __forceinline__ uint32_t band_row(const rt::TraceParams& P, uint32_t ly) {
    if (!P.rows) return P.off_y + ly;
    if (P.rows_lds != rt::kNoRowsLds)
        return reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(rt_dyn_lds) + P.rows_lds)[ly];
    return load_now(P.rows + ly);
}
// (before the prologue's barrier)
__device__ __forceinline__ void stage_rows(const rt::TraceParams& P, uint32_t tid, uint32_t nthr) {
    if (!P.rows || P.rows_lds == rt::kNoRowsLds) return;
    uint32_t* dst = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(rt_dyn_lds) + P.rows_lds);
    for (uint32_t i = tid; i < P.band_h; i += nthr) dst[i] = P.rows[i];
}

// shader.rgen:40 seed of pixel w (0..63) of 8x8 tile t of the band.
__device__ __forceinline__ uint32_t tile_pixel_seed(const rt::TraceParams& P, uint32_t t, uint32_t w) {
    const uint32_t lx = (t % P.tiles_x) * 8u + (w & 7u);
    const uint32_t ly = (t / P.tiles_x) * 8u + (w >> 3);
    const uint32_t gx = P.off_x + lx;
    const uint32_t gy = band_row(P, ly < P.band_h ? ly : P.band_h - 1u);   // ragged edge: unused
    return tea(tea(P.seed_local ? lx : gx, P.seed_local ? ly : gy), P.number);
}

// Block b's tile rank, chunk c and chunk count n: the head ranks' blocks come first, n =
// head_chunks, then the others', n = chunks (TraceParams). Chunk c of n runs samples
// [chunk_begin(c, n), chunk_begin(c + 1, n)); the host keeps n * spp below 2^32.
struct BlockChunk { uint32_t rank, c, n; };

__device__ __forceinline__ BlockChunk block_chunk(const rt::TraceParams& P, uint32_t b) {
    const uint32_t hb = P.head_tiles * P.head_chunks;
    if (b < hb) {
        const uint32_t rank = b / P.head_chunks;
        return BlockChunk{rank, b - rank * P.head_chunks, P.head_chunks};
    }
    const uint32_t b2 = b - hb, r2 = b2 / P.chunks;
    return BlockChunk{P.head_tiles + r2, b2 - r2 * P.chunks, P.chunks};
}

__device__ __forceinline__ uint32_t chunk_begin(const rt::TraceParams& P, uint32_t c, uint32_t n) {
    return (c * P.spp) / n;
}

// Unit hand-out. A wave takes whole 64-unit blocks (one chunk of one 8x8 tile, one atomic) from
// the device counter and gives their pixels to its lanes as they free, so a unit costs 1/64 of an
// atomic round trip and of a hand-out-order load instead of one each; the last units (>=
// n_block_units, the last 8 Ki) go out one by one. Per-pixel atomics on the one counter were the
// cost: 1080p at 13 spp took 10.5 ms with them, 4.8 ms with tiles (scripts/refill_ab.py).
// `blk` is wave-uniform: next unit and end of the wave's current block, its tile and chunk
// sample range; `dry` once the block phase is exhausted; `done` once the per-unit phase is
// exhausted too (later refills retire lanes without touching the counter: one address, every
// atomic on it queues behind the others). `seed` (per lane) is the pixel seed of the block's pixel
// `lane`: the 64 seeds of a tile are computed together when the block is taken (two TEAs, 16
// rounds each, with every lane busy) instead of one lane at a time as its unit starts.
struct WaveBlock {
    uint32_t next = 0, end = 0, tile = 0, s0 = 0, s1 = 0;
    bool dry = false, done = false;
    uint32_t seed = 0;
    // TAB == 2 kernels: the launch's n_units, n_block_units and first_blocks from the device record
    // TraceParams::tab_size (first_block); the other kernels read P's
    uint32_t n_units = 0, n_block_units = 0, first_blocks = 0;
};

__device__ __forceinline__ void take_block(const rt::TraceParams& P, uint32_t lane, WaveBlock& blk,
                                           uint32_t b, uint32_t tile) {
    const BlockChunk bc = block_chunk(P, b);
    blk.next = b * 64u;
    blk.end = blk.next + 64u;
    blk.tile = tile;
    blk.s0 = chunk_begin(P, bc.c, bc.n);
    blk.s1 = chunk_begin(P, bc.c + 1u, bc.n);
    blk.seed = tile_pixel_seed(P, tile, lane);
}

__device__ __forceinline__ uint32_t block_tile(const rt::TraceParams& P, uint32_t b) {
    const uint32_t rank = block_chunk(P, b).rank;
    return P.tile_order ? load_now(P.tile_order + rank) : rank;
}

// Table form (TAB kernels: HASH launches with a block table, rt_internal.h): block b (wave-uniform)
// is its table entry, one 16-byte load waited for at once where block_tile loads; the values are
// wave-uniform and go to SGPRs. Once per 64 units, outside the segment loop. The table form is a
// template parameter of the kernels, not a branch on P.block_tab: the branch cost the uniform
// launches 0.4 % of the headline.
__device__ __forceinline__ void take_block_tab(const rt::TraceParams& P, uint32_t lane, WaveBlock& blk, uint32_t b) {
    const rt::BlockEntry e = load_now_block(P.block_tab + b);
    blk.next = b * 64u;
    blk.end = blk.next + 64u;
    blk.tile = __builtin_amdgcn_readfirstlane(e.tile);
    blk.s0 = __builtin_amdgcn_readfirstlane(e.s0);
    blk.s1 = __builtin_amdgcn_readfirstlane(e.s1);
    blk.seed = tile_pixel_seed(P, blk.tile, lane);
}

template <int MODE>
__device__ __forceinline__ void begin_unit(const rt::TraceParams& P, Path& ps, uint32_t lx, uint32_t ly,
                                           uint32_t seed, uint32_t s0, uint32_t s1) {
    ps.px = lx | (ly << 16);
    ps.pixel_seed = seed;
    ps.seed = seed;
    ps.s = s0;
    ps.s_end = s1;
    ps.segs = 0;
    if constexpr (MODE == rt::MODE_FEATURES) {
        // -0 is the identity of binary32 addition (-0 + x = x for every x, a zero of either sign
        // included), so each sum starts from its first sample's value
        FeatPath& fp = feat_path(ps);
        fp.far = fp.fag = fp.fab = fp.fah = -0.0f;
        fp.fnx = fp.fny = fp.fnz = fp.fdz = -0.0f;
        return;
    }
    if (MODE == rt::MODE_HASH) {
        ps.qx = ps.qy = ps.qz = 0u;
    } else if (P.accumulate) {  // shader.rgen:53-55
        const float4 acc = load_now4(reinterpret_cast<const float4*>(P.accum) + size_t(ly) * P.band_w + lx);
        ps.sx = acc.x; ps.sy = acc.y; ps.sz = acc.z;
    } else {
        ps.sx = ps.sy = ps.sz = 0.0;
    }
}

// Tail stealing (counter-based stream only: any lane may run any sample of a pixel). Once the
// work queue is exhausted, a lane without work takes the upper half of the samples not yet started
// by the wave's lane with the most left (ties: lowest lane), one steal per call (one loop
// iteration), while the victim has at least 2 kStealMin left. The wave's last units are thus shared by its idle
// lanes instead of ending at the longest one; chunk sums are integers, so the split changes no bit.
constexpr uint32_t kStealMin = 4;

template <bool COUNT>
__device__ __forceinline__ void steal_tail(const rt::TraceParams& P, uint32_t lane, uint32_t& st, Path& ps) {
    const unsigned long long idle = __ballot(st == ST_RETIRED);
    if (!idle) return;
    const uint32_t rem = st == ST_TRACING ? ps.s_end - ps.s - 1u : st == ST_NEED_SAMPLE ? ps.s_end - ps.s : 0u;
    uint32_t key = (min(rem, (1u << 25) - 1u) << 6) | (63u - lane);
    for (int off = 32; off > 0; off >>= 1) key = max(key, (uint32_t)__shfl_xor(key, off));
    const uint32_t vrem = key >> 6;
    if (vrem < 2u * kStealMin) return;   // wave-uniform
    const int v = int(63u - (key & 63u));
    const int th = __ffsll(idle) - 1;
    const uint32_t k = vrem / 2u;
    const uint32_t vend = __shfl(ps.s_end, v), vpx = __shfl(ps.px, v), vseed = __shfl(ps.pixel_seed, v);
    if (int(lane) == v) ps.s_end -= k;
    if (COUNT && lane == 0) atomicAdd(&P.counters->steals, 1ull);
    if (int(lane) == th) {
        ps.px = vpx;
        ps.pixel_seed = vseed;
        ps.seed = vseed;
        ps.s = vend - k;
        ps.s_end = vend;
        ps.segs = 0;
        ps.qx = ps.qy = ps.qz = 0u;
        st = ST_NEED_SAMPLE;
    }
}

template <int MODE, bool COUNT, int TAB = 0>
__device__ __forceinline__ void refill(const rt::TraceParams& P, uint32_t lane, uint32_t& st, Path& ps,
                                       WaveBlock& blk, Stamps& stamps) {
    if (MODE == rt::MODE_HASH && blk.done) steal_tail<COUNT>(P, lane, st, ps);   // wave-uniform condition
    const unsigned long long need = __ballot(st == ST_NEED_UNIT);
    if (!need) return;
    STAMP(5);
    const uint32_t cnt = __popcll(need);
    const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
    const uint32_t avail = blk.end - blk.next;
    const int leader = __ffsll(need) - 1;
    uint32_t u = 0, t = 0, s0 = blk.s0, s1 = blk.s1;
    bool per_lane = false;
    uint32_t seed = __shfl(blk.seed, int((blk.next + rank) & 63u));   // all lanes: uniform control flow
    if (rank < avail) { u = blk.next + rank; t = blk.tile; }
    if (cnt <= avail) {
        blk.next += cnt;
    } else {
        STAMP(6);
        const uint32_t rest = cnt - avail;   // lanes beyond the current block's units
        uint32_t nb = 0xffffffffu;
        if (!blk.dry) {
            if (int(lane) == leader) nb = atomicAdd(&P.counters->work_head, 64u);
            nb = __builtin_amdgcn_readfirstlane(__shfl(nb, leader));
            if (nb >= (TAB == 2 ? blk.n_block_units : P.n_block_units)) blk.dry = true;
        }
        if (!blk.dry) {
            if (TAB) take_block_tab(P, lane, blk, nb >> 6);
            else take_block(P, lane, blk, nb >> 6, block_tile(P, nb >> 6));
            const uint32_t sn = __shfl(blk.seed, int((rank - avail) & 63u));
            if (rank >= avail) { u = nb + (rank - avail); t = blk.tile; seed = sn; s0 = blk.s0; s1 = blk.s1; }
            blk.next = nb + rest;
        } else {
            const uint32_t n_units = TAB == 2 ? blk.n_units : P.n_units;
            uint32_t tb = n_units;   // exhausted: the lanes retire
            if (!blk.done) {
                if (int(lane) == leader) tb = atomicAdd(&P.counters->work_tail, rest);
                tb = (TAB == 2 ? blk.n_block_units : P.n_block_units) + __shfl(tb, leader);
                if (tb + rest >= n_units) blk.done = true;
            }
            if (rank >= avail) { u = tb + (rank - avail); per_lane = true; }
            blk.next = blk.end;
        }
    }
    if (st != ST_NEED_UNIT) return;
    if (per_lane) {
        if (u >= (TAB == 2 ? blk.n_units : P.n_units)) { st = ST_RETIRED; return; }
        const uint32_t b = u >> 6;
        if (TAB) {   // entry u >> 6, per lane
            const rt::BlockEntry e = load_now_block(P.block_tab + b);
            t = e.tile;
            s0 = e.s0;
            s1 = e.s1;
        } else {
            const BlockChunk bc = block_chunk(P, b);
            t = P.tile_order ? load_now(P.tile_order + bc.rank) : bc.rank;
            s0 = chunk_begin(P, bc.c, bc.n);
            s1 = chunk_begin(P, bc.c + 1u, bc.n);
        }
    }
    const uint32_t w = u & 63u;
    const uint32_t lx = (t % P.tiles_x) * 8u + (w & 7u);
    const uint32_t ly = (t / P.tiles_x) * 8u + (w >> 3);
    if (lx >= P.band_w || ly >= P.band_h) return;   // ragged edge: stays NEED_UNIT, refetches
    if (per_lane) seed = tile_pixel_seed(P, t, w);
    begin_unit<MODE>(P, ps, lx, ly, seed, s0, s1);
    st = ST_NEED_SAMPLE;
}

// First block of a wave: by wave id, not through the counter (the host starts the counter past
// them): 16 Ki waves asking one address at once would queue for ~0.1 ms. Block ranks are dealt
// across blocks of the grid first (rank = wave-in-block * grid + block), so the longest chains of
// the LPT order start on different CUs (and XCDs) instead of sharing block 0's SIMDs.
template <int TAB = 0>
__device__ __forceinline__ void first_block(const rt::TraceParams& P, uint32_t lane, WaveBlock& blk) {
    const uint32_t wid = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
    uint32_t first_blocks = P.first_blocks;
    if (TAB == 2) {
        // A table planned on the device: the launch's sizes are a 16-byte device
        // record, written before the launch on its stream, read here once per wave; wave-uniform, to
        // SGPRs. The grid is the full persistent grid then, whatever the table holds: a wave past
        // first_blocks starts without a block and asks the counters as any wave does after its first
        // block, so an empty table (every size 0) retires every lane at its first refill.
        const rt::BlockEntry z = load_now_block(reinterpret_cast<const rt::BlockEntry*>(P.tab_size));
        blk.n_units = __builtin_amdgcn_readfirstlane(z.tile);
        blk.n_block_units = __builtin_amdgcn_readfirstlane(z.s0);
        first_blocks = blk.first_blocks = __builtin_amdgcn_readfirstlane(z.s1);
    }
    if (wid < first_blocks) {
        if (TAB) take_block_tab(P, lane, blk, wid);
        else take_block(P, lane, blk, wid, block_tile(P, wid));
        if (wid < P.isolate_blocks) blk.dry = blk.done = true;   // no work beyond its first block
    }
}

// shader.rgen:61-66: store the finished pixel (dvec3 sum rounded to float, rgba8 resolve).
__device__ __forceinline__ void store_pixel(const rt::TraceParams& P, const Path& ps) {
    const uint32_t lx = ps.px & 0xffffu, ly = ps.px >> 16;
    const float s0 = float(ps.sx), s1 = float(ps.sy), s2 = float(ps.sz);
    const size_t texel = size_t(ly) * P.band_w + lx;
    reinterpret_cast<float4*>(P.accum)[texel] = make_float4(s0, s1, s2, 1.0f);
    const float spp = float(P.spp);
    const uint32_t r8 = unorm8(__builtin_sqrtf(s0 / spp));
    const uint32_t g8 = unorm8(__builtin_sqrtf(s1 / spp));
    const uint32_t b8 = unorm8(__builtin_sqrtf(s2 / spp));
    P.out[texel] = r8 | (g8 << 8) | (b8 << 16) | (255u << 24);
}

// Finished unit. STREAM: the unit is the whole pixel: store it. HASH: flush the chunk's remaining
// partial fixed-point sum.
template <int MODE, bool LSUM>
__device__ __forceinline__ void finish_unit(const rt::TraceParams& P, Path& ps) {
    if constexpr (MODE == rt::MODE_PROBE) return;   // the ray's record is already stored (shade_rec)
    if constexpr (MODE == rt::MODE_FEATURES) {      // the pixel's two feature texels (shade_rec summed them)
        const size_t texel = size_t(ps.px >> 16) * P.band_w + (ps.px & 0xffffu);
        const FeatPath& fp = feat_path(ps);
        reinterpret_cast<float4*>(P.feat0)[texel] = make_float4(fp.far, fp.fag, fp.fab, fp.fah);
        reinterpret_cast<float4*>(P.feat1)[texel] = make_float4(fp.fnx, fp.fny, fp.fnz, fp.fdz);
        return;
    }
    if (MODE == rt::MODE_HASH && LSUM) {   // the unit's whole sum from LDS, once
        unsigned long long* s = lane_sum_slot();
        const unsigned long long x = s[0] + ps.qx, y = s[RT_TRACE_BLOCK] + ps.qy, z = s[2 * RT_TRACE_BLOCK] + ps.qz;
        if (x | y | z) add_fixed(P, ps, x, y, z);
        s[0] = s[RT_TRACE_BLOCK] = s[2 * RT_TRACE_BLOCK] = 0ull;
        ps.qx = ps.qy = ps.qz = 0u;
    } else if (MODE == rt::MODE_HASH) {
        if (ps.qx | ps.qy | ps.qz) flush_fixed<false>(P, ps);
    } else {
        store_pixel(P, ps);
    }
}

// Finished unit: its chain length (traced segments) feeds the next launch's hand-out order. HASH:
// only the units of the tile's 16 pixels with even coordinates record (a quarter of the
// memory-side atomic requests; the image does not depend on the order); STREAM: every pixel, the
// frame ends with the longest chain.
template <int MODE>
__device__ __forceinline__ void record_tile_cost(const rt::TraceParams& P, const Path& ps) {
    // (P.tile_cost is set for every walk kernel, the only callers; a probe launch has none and leaves
    // the context's LPT record alone)
    if constexpr (MODE == rt::MODE_PROBE || MODE == rt::MODE_FEATURES) return;
    if (MODE == rt::MODE_HASH && (ps.px & 0x00010001u)) return;
    const uint32_t lx = ps.px & 0xffffu, ly = ps.px >> 16;
    uint32_t* c = &P.tile_cost[(ly >> 3) * P.tiles_x + (lx >> 3)];
#ifdef RT_TILE_COST_SUM   // A/B build: order tiles by their summed chains instead
    atomicAdd(c, ps.segs);
#else
    atomicMax(c, ps.segs);
#endif
}

}  // namespace
