// rt_trace_batch.h — the camera-batch form of the segment loop (device only): a
// wave works on one block (one 8x8 tile, samples [s0, s1)) at a time. The camera rays of one sample
// index of the tile's 64 pixels are traced together as one full wave (a generation batch: lane i =
// pixel i, shaders/shader.rgen:56-58 + the first bounce-loop step :77-88); the paths that survive
// their camera segment wait in a per-wave queue in LDS, and the bounce loop traces only bounce
// segments, each lane popping its next path from the queue as its path ends. The counter-based
// stream makes this exact: every sample has its own LCG start and the pixel sums are integers, so
// the samples of a pixel may run in any order on any lane without changing a bit.
// No reference counterpart beyond the lines named: the reference runs one invocation per pixel.
//
// Per wave in LDS: the block's 64 x 3 pixel sums (u64, s_lane_sum's slots, one per pixel instead of
// one per lane), 64 chain counters (the pixel's traced segments in this block, the tile-cost record)
// and the queue of kBatchQueue entries {o, LCG state | d, word}, word = pixel | alt << 6 | bi << 7.
// Nothing is shared between waves beyond what the unit loop shares (the work counter, the HBM sums,
// the tile-cost record), no lane waits for another lane or wave, and the LDS is wave-synchronous:
// ranks come from ballots, and lane_order() keeps the compiler from reordering what different lanes
// write and read.
//
// A queue entry holds no thr. Only generation batches write the queue, so every entry is a path of
// depth 1 whose thr is mul((1, 1, 1), att) of its first hit (shade_rec), att = m0.rgb of sphere bi,
// or m1.rgb where the checker texture chose colour 1 (alt): the pop loads mat4[2 bi + alt] and takes
// its rgb. That is the same bits: the form runs HASH launches only, which the library refuses unless
// every colour att can be lies in [0, 1] (colours_in_unit: NaN, infinities and values above 1 fail;
// a colors[1] outside [0, 1] is accepted only where no texture reads it, and then alt = 0). For
// every binary32 x in [0, 1], 1.0f * x is x bit for bit: the product is exact, so it is x for
// normal and denormal x alike (f32 denormals are not flushed: the build sets no flush flag and the
// unit loop and the CPU oracle multiply them the same way), and (+1) * (+-0) is +-0. bi is at most
// kRecStatic - 1 = 511 (the form's ACCEL_GRID_REC condition), so the word has room to spare.
//
// Block-wide in LDS, staged before the kernel's barrier and read-only after it: the winner's gate
// records s_gate[bi] = {cx, cy, cz, r} (one ds_read_b128 for the gate and shading's centre; the two
// material records still come from L2, requested before the gate and first used in shading) and the
// camera-origin terms of a generation batch (rt_trace_prims.h s_cam_tab).
#pragma once

#include <assert.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_grid.h"
#include "rt_trace_prims.h"
#include "rt_trace_shade.h"
#include "rt_trace_units.h"
#include "rt_trace_walk.h"

using namespace rtd;

namespace {

__shared__ uint32_t s_pix_chain[RT_TRACE_BLOCK];
__shared__ float4 s_q_o[RT_TRACE_BLOCK];        // o.xyz, LCG state
__shared__ float4 s_q_d[RT_TRACE_BLOCK];        // d.xyz (normalised), word
static_assert(rt::kBatchQueue == 64u, "one queue slot per lane of a wave: slot = wave0 + entry");
constexpr bool kGateLds = RT_BATCH_GATE_LDS != 0, kCameraTerms = RT_BATCH_CAMERA_TERMS != 0;
constexpr bool kLeanHit = RT_BATCH_LEAN_HIT != 0;
#if RT_BATCH_GATE_LDS
// The winner's gate records by sphere id, {cx, cy, cz, r}: static, so a record's address is 16 bi
// with no base register (DESIGN.md §4.8 measured what a spilled table base costs). Without the
// camera terms (A/B build) their 1 KB stays here as spare, so the form's LDS is the same.
__shared__ float4 s_gate[rt::kBatchGateRecs + (RT_BATCH_CAMERA_TERMS ? 0u : rt::kBatchCamTabBytes / 16u)];
static_assert(sizeof(s_pix_chain) + sizeof(s_q_o) + sizeof(s_q_d) + sizeof(s_gate) +
                      (kCameraTerms ? sizeof(s_cam_tab) : 0u) == rt::kBatchLdsBytes, "rt_internal.h");
static_assert(rt::kBatchLdsBytes == 36864u, "rt_launch.h kBatchStaticLdsBytes: 55 408 B, pinned by the plan's tests");
#else   // A/B build: the 44-byte entry with its thr, the gate's records from L2
__shared__ float s_q_thr[3 * RT_TRACE_BLOCK];   // thr.x | thr.y | thr.z planes
static_assert(sizeof(s_pix_chain) + sizeof(s_q_o) + sizeof(s_q_d) + sizeof(s_q_thr) +
                      (kCameraTerms ? sizeof(s_cam_tab) : 0u) == rt::kBatchLdsBytes, "rt_internal.h");
#endif

// Before the kernel's first barrier: the gate table (the form runs only where n_spheres <=
// kRecStatic, rt_launch.cpp; the min keeps any other launch inside the table) ...
__device__ __forceinline__ void stage_gate(const rt::TraceParams& P, uint32_t tid, uint32_t nthr) {
#if RT_BATCH_GATE_LDS
    const uint32_t n = min(P.n_spheres, rt::kBatchGateRecs);
    for (uint32_t i = tid; i < n; i += nthr) {
        const rt::GeomRec g = P.geom[i];
        s_gate[i] = make_float4(g.cx, g.cy, g.cz, P.radius[i]);
    }
#endif
}
// ... and the camera-origin terms (s_cam_tab), computed here on the device by big_group's and
// grid_walk's own expressions on cam.lf (load_camera's P.lf), never on the host, whose
// floating-point contraction is not the kernel's. The big-sphere table always holds four records
// (rt_launch_prep_kernel: the first four, padded by repeating the last, or four inert ones).
__device__ __forceinline__ void stage_camera_terms(const rt::TraceParams& P, uint32_t tid) {
    if constexpr (!kCameraTerms) return;
    if (tid < 4u) {
        const float* sb = P.big_tab + 4u * tid;
        const float rr = sb[3] * sb[3];
        const float ocx = P.lf[0] - sb[0], ocy = P.lf[1] - sb[1], ocz = P.lf[2] - sb[2];
        const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
        s_cam_tab[tid] = make_float4(ocx, ocy, ocz, c);
    } else if (tid < 7u) {
        const uint32_t k = tid - 4u;
        s_cam_tab[tid] = make_float4(P.grid.lo_m[k] - P.lf[k], P.grid.hi_m[k] - P.lf[k], P.grid.inv_cs[k],
                                     __uint_as_float(P.grid.n[k] - 1u));
    }
}

// A path's colour and chain length added to its pixel (return-less LDS atomics: lanes of the wave
// may end paths of the same pixel in one pass).
__device__ __forceinline__ void batch_path_end(uint32_t wave0, uint32_t pix, const Path& t, uint32_t segs) {
    unsigned long long* s = s_lane_sum + wave0 + pix;
    __hip_atomic_fetch_add(s, (unsigned long long)t.qx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_fetch_add(s + RT_TRACE_BLOCK, (unsigned long long)t.qy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_fetch_add(s + 2 * RT_TRACE_BLOCK, (unsigned long long)t.qz, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_fetch_add(s_pix_chain + wave0 + pix, segs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// One segment of every lane with `active` (the whole wave takes part: setup_ray and the regate are
// wave-wide), the unit loop's steps in its order: ray setup, grid walk, the winner's gate, shading.
// t holds the path's LCG state, depth and thr; it is shaded as a one-sample unit (s = 0, s_end = 1),
// so shade_rec itself ends the sample: false = the path ended and t.q{x,y,z} hold its colour; true
// = r.o, r.d hold the next segment's ray.
// CAMERA: a generation batch. Every active lane's ray starts at cam.lf (or at NaN), so the setup and
// the grid entry take their origin terms from s_cam_tab, and alt reports the checker's choice of
// the first hit (1: colour 1), which with r.bi names the material record the path's thr is.
template <bool FLAT, bool CAMERA>
__device__ __forceinline__ bool batch_segment(const rt::TraceParams& P, const Camera& cam,
                                              const float4* __restrict__ cst, const float4* __restrict__ refs,
                                              const uint32_t* __restrict__ ids, const float4* __restrict__ geom4,
                                              const float4* __restrict__ mat4, uint32_t lane, bool active, Ray& r,
                                              Path& t, uint32_t& alt) {
    constexpr bool CAM = CAMERA && kCameraTerms;
    uint32_t n_box = 0, n_sph = 0, n_empty = 0;
    __builtin_amdgcn_s_setprio(1);   // (the unit loop's window: ray setup to the winner's records)
    setup_ray<false, CAM>(P, r);
    r.walk = true;
    if (active) walk<false, LAYOUT_GRID, FLAT, CAM>(P, cst, refs, ids, r, n_box, n_sph, n_empty);
    // LEAN: the record has no value in a lane that loaded none, and the gate's verdict is formed where
    // the record was loaded, so no lane reads (or zeroes) a record it does not have: twelve moves
    // per segment less, and fewer registers live across the branch
    HitRec hr;
    bool gate_fail = false;
    [[maybe_unused]] float rad0 = 0.0f;
    if constexpr (!kLeanHit) hr = HitRec{};
    if (active && r.bi != 0xffffffffu) {
        float rad;
        if constexpr (kGateLds) {
            // the material records from L2, requested first and not waited for before shading; the
            // gate's record from LDS (shading reads its centre only, so w may hold r)
            hr.m0 = mat4[2 * r.bi];
            hr.m1 = mat4[2 * r.bi + 1];
#if RT_BATCH_GATE_LDS
            hr.g = s_gate[r.bi];
#endif
            rad = hr.g.w;
        } else {
            hr = load_hit(geom4, mat4, r.bi);
            rad = P.radius[r.bi];
        }
        if constexpr (kLeanHit) gate_fail = !aabb_hit(hr.g.x, hr.g.y, hr.g.z, rad, r.o, r.inv);
        else rad0 = rad;
    }
    if constexpr (!kLeanHit)   // (A/B build: every lane gates the record it has or the zeroed one)
        gate_fail = active && r.bi != 0xffffffffu && !aabb_hit(hr.g.x, hr.g.y, hr.g.z, rad0, r.o, r.inv);
    unsigned long long regate = __ballot(gate_fail);
    if (P.force_regate) regate = __ballot(active);
    if (__builtin_expect(regate != 0ull, 0)) {
        regate_brute<false>(P, geom4, lane, regate, r);
        if (((regate >> lane) & 1ull) && r.bi != 0xffffffffu) hr = load_hit(geom4, mat4, r.bi);
    }
    __builtin_amdgcn_s_setprio(0);
    bool more = false, fresh = false;
    if (active) {
        t.s = 0u;
        t.s_end = 1u;
        t.qx = t.qy = t.qz = 0u;
        if constexpr (CAMERA && kGateLds) {
            alt = 0u;
            more = shade_rec<rt::MODE_HASH, true, true, true, kLeanHit>(P, cam, hr, t, r.bi, r.best, r.o, r.d, fresh, &alt);
        } else {
            more = shade_rec<rt::MODE_HASH, true, true, false, kLeanHit>(P, cam, hr, t, r.bi, r.best, r.o, r.d, fresh);
        }
    }
    return more;
}

// The loop. cst / refs / ids: the grid staged in LDS (rt_trace_grid_kernel's layout); geom4 / mat4:
// the scene's records in HBM (through L2: shading's material records, a popped path's thr, and the
// geometry of the rare regate).
//
// Termination: every iteration does exactly one of four things.
//   (a) batch:  some lane is idle after the queue was handed out (so the queue is empty) and s < s1:
//               sample s of the tile is traced, s advances. At most s1 - s0 per block.
//   (b) block:  no lane holds a path (so the queue is empty too) and s == s1: the block is flushed
//               and the next one taken from the work counter, or the loop exits when there is none.
//   (c) trace:  otherwise at least one lane holds a path: every such lane traces one segment; a path
//               has at most max_depth segments, and only (a) makes paths.
//   (d) exit:   inside (b).
// Nothing waits: no iteration depends on another wave, and lanes of the wave run in lockstep.
template <bool FLAT>
__device__ __forceinline__ void batch_loop(const rt::TraceParams& P, const float4* __restrict__ cst,
                                           const float4* __restrict__ refs, const uint32_t* __restrict__ ids,
                                           const float4* __restrict__ geom4, const float4* __restrict__ mat4) {
    const uint32_t lane = lane_id();
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    const Camera cam = load_camera(P);
    {   // this wave's slots (written and read by this wave only: no barrier)
        unsigned long long* z = s_lane_sum + wave0 + lane;
        z[0] = z[RT_TRACE_BLOCK] = z[2 * RT_TRACE_BLOCK] = 0ull;
        s_pix_chain[wave0 + lane] = 0u;
        lane_order();
    }
    uint32_t seg_w = 0, smp_w = 0;   // wave-uniform: ballot counts
    WaveBlock blk;
    first_block<0>(P, lane, blk);
    if (lane == 0) atomicMin(&P.counters->t_first, __builtin_amdgcn_s_memrealtime());
    bool have = blk.end != blk.next;   // a first block by wave id
    // the next block from the work counter: whole blocks only, up to n_units (this form has no
    // one-by-one reserve; the counter starts past the first blocks)
    auto take = [&]() -> bool {
        if (blk.dry) return false;
        uint32_t nb = 0u;
        if (lane == 0) nb = atomicAdd(&P.counters->work_head, 64u);
        nb = __builtin_amdgcn_readfirstlane(nb);
        if (nb >= P.n_units) {   // this wave saw the queue run dry
            blk.dry = true;
            if (lane == 0) atomicMin(&P.counters->t_dry, __builtin_amdgcn_s_memrealtime());
            return false;
        }
        take_block(P, lane, blk, nb >> 6, block_tile(P, nb >> 6));
        return true;
    };
    if (!have) have = take();
    // the wave's state: next sample index of the block and queue length (wave-uniform); per lane its
    // pixel of the block (px; valid: inside the band) and the path it holds (live: r.o, r.d, t.seed,
    // t.thr, word = pixel | depth << 6)
    uint32_t s = blk.s0, qn = 0u, px = 0u, word = 0u;
    bool valid = false, live = false;
    Ray r{};
    r.d = v3(0.0f, 0.0f, 1.0f);
    Path t{};
    auto block_pixels = [&]() {
        const uint32_t lx = (blk.tile % P.tiles_x) * 8u + (lane & 7u);
        const uint32_t ly = (blk.tile / P.tiles_x) * 8u + (lane >> 3);
        valid = lx < P.band_w && ly < P.band_h;   // ragged edge: the lane generates nothing
        px = lx | (ly << 16);
        s = blk.s0;
    };
    if (have) block_pixels();
    while (have) {
        // idle lanes take the queue's last entries
        const unsigned long long idle = __ballot(!live);
        if (idle && qn) {
            const uint32_t n = min(uint32_t(__popcll(idle)), qn);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(idle >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(idle), 0u));
            if (!live && rank < n) {
                const uint32_t e = wave0 + (qn - 1u - rank);
                const float4 a = s_q_o[e], b = s_q_d[e];
                r.o = v3(a.x, a.y, a.z);
                r.d = v3(b.x, b.y, b.z);
                t.seed = __float_as_uint(a.w);
                const uint32_t w = __float_as_uint(b.w);
#if RT_BATCH_GATE_LDS
                // thr = the rgb of material record 2 bi + alt (the header's argument): one 16-byte
                // load from L2, requested here and first needed in the path's next shading. Every
                // entry has depth 1.
                const float4 m = mat4[w >> 6];
                t.thr = v3(m.x, m.y, m.z);
                word = (w & 63u) | (1u << 6);
#else
                word = w;
                t.thr = v3(s_q_thr[e], s_q_thr[RT_TRACE_BLOCK + e], s_q_thr[2 * RT_TRACE_BLOCK + e]);
#endif
                live = true;
            }
            qn -= n;
            lane_order();
        }
        const unsigned long long tracing = __ballot(live);
        if (~tracing != 0ull && s < blk.s1) {
            // (a) a generation batch: lane i traces sample s of pixel i; lanes holding a path keep it
            // in their registers. The queue is empty here: the survivors become entries 0 .. n - 1.
            Path c{};
            Ray rc{};
            rc.d = v3(0.0f, 0.0f, 1.0f);
            if (valid) {
                c.px = px;
                c.pixel_seed = blk.seed;
                c.s = s;
                V3 v;
                camera_ray<rt::MODE_HASH, true>(P, cam, c, rc.o, v);
                rc.d = normalize(v);
            }
            uint32_t alt = 0u;
            const bool more = batch_segment<FLAT, true>(P, cam, cst, refs, ids, geom4, mat4, lane, valid, rc, c, alt);
            const uint32_t n_valid = __popcll(__ballot(valid));
            seg_w += n_valid;
            smp_w += n_valid;
            if (valid && !more) batch_path_end(wave0, lane, c, 1u);
            const unsigned long long surv = __ballot(valid && more);
            if (valid && more) {
                const uint32_t e = wave0 + __builtin_amdgcn_mbcnt_hi(uint32_t(surv >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(surv), 0u));
                s_q_o[e] = make_float4(rc.o.x, rc.o.y, rc.o.z, __uint_as_float(c.seed));
#if RT_BATCH_GATE_LDS
                // a survivor scattered at its camera segment's hit (shade_rec returns true from its
                // scatter branch alone here: the unit has one sample): depth 0 -> 1, bi a sphere id.
                // Checked in -DRT_BATCH_ASSERT builds only: the compiler does not fold the test
                // away, and a device assert raises this kernel's scratch from 44 to 112 B per lane.
#ifdef RT_BATCH_ASSERT
                assert(c.depth == 1u && rc.bi < rt::kBatchGateRecs);
#endif
                s_q_d[e] = make_float4(rc.d.x, rc.d.y, rc.d.z, __uint_as_float(lane | (alt << 6) | (rc.bi << 7)));
#else
                s_q_d[e] = make_float4(rc.d.x, rc.d.y, rc.d.z, __uint_as_float(lane | (c.depth << 6)));
                s_q_thr[e] = c.thr.x;
                s_q_thr[RT_TRACE_BLOCK + e] = c.thr.y;
                s_q_thr[2 * RT_TRACE_BLOCK + e] = c.thr.z;
#endif
            }
            qn = __popcll(surv);
            lane_order();
            s++;
            continue;
        }
        if (!tracing) {
            // (b) the block is done: its pixel sums to HBM (all-zero sums skipped), its tile-cost
            // record by the unit loop's rule (a pixel's summed segments in this block, the pixels
            // with even coordinates only), then the next block
            lane_order();
            unsigned long long* z = s_lane_sum + wave0 + lane;
            const unsigned long long x = z[0], y = z[RT_TRACE_BLOCK], w = z[2 * RT_TRACE_BLOCK];
            const uint32_t chain = s_pix_chain[wave0 + lane];
            z[0] = z[RT_TRACE_BLOCK] = z[2 * RT_TRACE_BLOCK] = 0ull;
            s_pix_chain[wave0 + lane] = 0u;
            lane_order();
            if (valid) {
                Path f{};
                f.px = px;
                f.segs = chain;
                if (x | y | w) add_fixed(P, f, x, y, w);
                record_tile_cost<rt::MODE_HASH>(P, f);
            }
            have = take();
            if (have) block_pixels();
            continue;
        }
        // (c) one bounce segment of every lane that holds a path
        seg_w += __popcll(tracing);
        t.depth = word >> 6;
        uint32_t unused = 0u;
        const bool more = batch_segment<FLAT, false>(P, cam, cst, refs, ids, geom4, mat4, lane, live, r, t, unused);
        if (live) {
            if (more) {
                word = (word & 63u) | (t.depth << 6);
            } else {
                batch_path_end(wave0, word & 63u, t, (word >> 6) + 1u);
                live = false;
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&P.counters->segments, (unsigned long long)seg_w);
        atomicAdd(&P.counters->samples, (unsigned long long)smp_w);
        atomicMax(&P.counters->t_last, __builtin_amdgcn_s_memrealtime());
    }
}

}  // namespace
