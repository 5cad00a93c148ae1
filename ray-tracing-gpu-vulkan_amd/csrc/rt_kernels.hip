// rt_kernels.hip — the MI355X path-tracing hot path (hand-written HIP for gfx950).
//
// One fused persistent kernel replaces the reference's whole ray-tracing pipeline:
//   shaders/shader.rgen   per-pixel seed, sample loop, camera ray, depth-50 bounce loop,
//                         sample accumulation, accumulator store and rgba8 tonemap
//   shaders/shader.rint   ray-sphere quadratic, t1-else-t2 report inside [tmin, tmax]
//   driver traversal      closest hit: brute force (sphere list through the scalar cache) or a
//                         stackless LBVH walk (node copies in LDS, or an LDS treelet over L2)
//   shaders/shader.rchit  normal, texture, diffuse / metal / dielectric scatter
//   shaders/shader.rmiss  constant sky
//
// Execution model: a lane owns one work unit — a chunk of one pixel's samples
// (the whole pixel in the reference's per-pixel LCG stream mode, whose samples are one sequential
// chain) — flattened into one `segment` loop: every iteration traces one segment for every active
// lane; a lane whose sample ends starts the next sample of its unit, a lane whose unit ends takes
// a new one. A wave takes units 64 at a time (one chunk of one 8x8 tile) from a device-wide
// counter, longest tiles first, and hands them to its lanes as they free (ranks from the ballot),
// so lanes stay busy under divergent bounce depth until the image runs out of work.
//
// This file holds the segment loop and the five __global__ trace kernels with their launcher. What
// they are made of is in the device-only headers beside it (map of the kernel sources).
#include <hip/hip_runtime.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_launchers.h"
#include "rt_trace_diag.h"
#include "rt_trace_prims.h"
#include "rt_trace_units.h"
#include "rt_trace_shade.h"
#include "rt_trace_walk.h"
#include "rt_trace_grid_coop.h"
#include "rt_trace_batch.h"

using namespace rtd;

namespace {

// Waves per SIMD the register budget is sized for. Brute force: 6 (71 VGPRs, no spills). LBVH:
// 6 (80 VGPRs) in 768-thread blocks (12 waves, 3 per SIMD), two blocks per CU: the staged octant
// tree (73 KB) and the depth-10 treelet (64 KB) fit twice in the 160 KB LDS. Measured at 1080p /
// 1000 spp (scripts/perf_variants.py): 165 ms against 193 ms for one 1024-thread
// block per CU at 4 waves per SIMD (98 VGPRs), although the 80-VGPR budget spills ~31 VGPRs
// outside the walk loop; 8 waves per SIMD (64 VGPRs) spill more and took 180 ms; blocks whose
// wave count is not a multiple of 4 (640, 896 threads) leave SIMDs unevenly loaded (+50 %).
#ifndef RT_BRUTE_WAVES_PER_SIMD
#define RT_BRUTE_WAVES_PER_SIMD 6
#endif
#ifndef RT_TRACE_WAVES_PER_SIMD
#define RT_TRACE_WAVES_PER_SIMD 6
#endif
constexpr uint32_t kBruteBlock = 256;
constexpr uint32_t kTraceBlock = RT_TRACE_BLOCK;   // one block per CU shares one staged tree / treelet

// ---------------------------------------------------------------------------------------------
// Brute-force kernel: one segment per loop iteration for every lane (the sphere loop is
// wave-uniform, so there is no traversal divergence to manage).
// ---------------------------------------------------------------------------------------------
template <bool COUNT, int MODE, int TAB = 0>
__global__ __launch_bounds__(kBruteBlock, RT_BRUTE_WAVES_PER_SIMD) void rt_trace_brute_kernel(const rt::TraceParams P) {
    const uint32_t lane = lane_id();
    const Camera cam = load_camera(P);
    uint32_t st = ST_NEED_UNIT;
    PathOf<MODE> ps{};
    V3 o = v3(0, 0, 0), d = v3(0, 0, 1);
    uint32_t n_seg = 0, n_smp = 0, n_sph = 0;
    WaveBlock blk;
    first_block<TAB>(P, lane, blk);
    STAMP_DECL;
    for (;;) {
        refill<MODE, COUNT, TAB>(P, lane, st, ps, blk, stamps);
        if (st == ST_NEED_SAMPLE) {
            if (start_sample<MODE, false>(P, cam, ps, o, d)) { st = ST_TRACING; n_smp++; }
            else st = ST_NEED_UNIT;
        }
        if (__ballot(st == ST_NEED_UNIT)) continue;   // refill before the next trace
        if (!__ballot(st == ST_TRACING)) break;        // every lane retired
        if (st == ST_TRACING) {
            float best = T_MAX_SUCC;
            uint32_t bi = 0xffffffffu;
            const V3 inv = v3(rcp_cr(d.x), rcp_cr(d.y), rcp_cr(d.z));
            const float a = dot(d, d);
            const float ia = rcp_cr(a);
            // AABB gate of the winner only: the ungated minimum is the
            // gated one when it passes; otherwise the gated pass (rare, one lane's own cost)
            closest_brute<false>(P, o, d, inv, a, ia, best, bi);
            if (bi != 0xffffffffu) {
                const float4 g = reinterpret_cast<const float4*>(P.geom)[bi];
                if (!aabb_hit(g.x, g.y, g.z, P.radius[bi], o, inv)) {
                    best = T_MAX_SUCC;
                    bi = 0xffffffffu;
                    closest_brute<true>(P, o, d, inv, a, ia, best, bi);
                }
            }
            if (COUNT) n_sph += P.n_spheres;
            n_seg++;
            ps.segs++;
            bool fresh = false;
            if (!shade<MODE, false>(P, cam, reinterpret_cast<const float4*>(P.geom),
                                    reinterpret_cast<const float4*>(P.mat), ps, bi, best, o, d, fresh)) {
                finish_unit<MODE, false>(P, ps);
                st = ST_NEED_UNIT;
            }
            if (fresh) n_smp++;
        }
    }
    atomicAdd(&P.counters->segments, (unsigned long long)n_seg);
    atomicAdd(&P.counters->samples, (unsigned long long)n_smp);
    if (COUNT) atomicAdd(&P.counters->sphere_tests, (unsigned long long)n_sph);
}

// ---------------------------------------------------------------------------------------------
// LBVH segment loop: one segment per lane per loop iteration; the wave's walk runs until its
// longest walk ends. Stamp slots: 0 loop head, 4 sample start, 5 refill, 6 block fetch, 1 ray
// setup (big spheres), 2 LBVH walk, 3 shading, 7 other.
// ---------------------------------------------------------------------------------------------
template <bool COUNT, int LAYOUT, int MODE, bool REC = false, bool FLAT = false, int TAB = 0>
__device__ __forceinline__ void lbvh_loop(const rt::TraceParams& P, const float4* __restrict__ nodes4,
                                          const float4* __restrict__ leaf4,
                                          const uint32_t* __restrict__ leaf_ids,
                                          const float4* __restrict__ geom4, const float4* __restrict__ mat4) {
    // the one-layer L2 grid kernel (config 5's) also takes pinhole_lf and at most four big spheres
    // as compile-time facts (flat_grid_form: the host proves both): no camera test and no further
    // big-sphere groups in its segment loop (config 5 -0.5 %; the same for the LDS kernels measured
    // +0.64 % on config 3)
    constexpr bool SPEC = FLAT && LAYOUT == LAYOUT_GRID_L2;
    constexpr bool LSUM = MODE == rt::MODE_HASH &&
                          (LAYOUT == LAYOUT_GRID || LAYOUT == LAYOUT_GRID_L2 || LAYOUT == LAYOUT_GRID_COOP ||
                           LAYOUT == LAYOUT_GRID_CQ);
    const uint32_t lane = lane_id();
    const Camera cam = load_camera(P);
    uint32_t st = ST_NEED_UNIT;
    PathOf<MODE> ps{};
    Ray r{};
    if (LSUM) {   // this thread's unit sums (read and written by this thread only: no barrier)
        unsigned long long* s = lane_sum_slot();
        s[0] = s[RT_TRACE_BLOCK] = s[2 * RT_TRACE_BLOCK] = 0ull;
    }
    // traced segments and started samples of this wave (wave-uniform: ballot counts, no per-lane
    // registers); per-lane test counters in COUNT builds only
    uint32_t seg_w = 0, smp_w = 0, n_box = 0, n_sph = 0, n_empty = 0;
    unsigned long long wave_iters = 0;
    bool saw_dry = false;
    WaveBlock blk;
    first_block<TAB>(P, lane, blk);
    // launch telemetry (3 atomics per wave): first start, work queue dry, last exit
    if (lane == 0) atomicMin(&P.counters->t_first, __builtin_amdgcn_s_memrealtime());
    STAMP_DECL;
    for (;;) {
        STAMP(0);
        refill<MODE, COUNT, TAB>(P, lane, st, ps, blk, stamps);
        if (!saw_dry && __ballot(st == ST_RETIRED)) {   // this wave saw the queue run dry
            saw_dry = true;
            if (lane == 0) atomicMin(&P.counters->t_dry, __builtin_amdgcn_s_memrealtime());
        }
        STAMP(4);
        bool started = false;
        if (st == ST_NEED_SAMPLE) {
            if (start_sample<MODE, LSUM, SPEC>(P, cam, ps, r.o, r.d)) {
                st = ST_TRACING;
                started = true;
            } else {   // empty unit (spp = 0): stored at once
                st = ST_NEED_UNIT;
                record_tile_cost<MODE>(P, ps);
            }
        }
        smp_w += __popcll(__ballot(started));
        if (__ballot(st == ST_NEED_UNIT)) continue;   // refill before the next trace
        const unsigned long long tracing = __ballot(st == ST_TRACING);
        if (!tracing) break;                           // every lane retired
        seg_w += __popcll(tracing);
        if (COUNT && lane == 0) atomicAdd(&P.counters->lane_hist[__popcll(tracing)], 1ull);
        STAMP(1);
        UTIL(8, st == ST_TRACING);
        const uint32_t box0 = n_box;
        // Wave priority 1 from the ray setup to the winner's records (the segment's dependent
        // L2 / LDS round trips), 0 in shading and refill: on a SIMD the waves waiting on the walk
        // issue their next load ahead of the ones in shading's long VALU runs. Config 3 -0.5 %,
        // reference stream -4.2 %, config 5 -1.1 % (profiles/r06t_ab_*).
        __builtin_amdgcn_s_setprio(1);
        // every lane (a lane that is not tracing computes on its last ray and discards the result):
        // inside a per-lane branch the big-sphere loop's launch-uniform bound became a spilled lane mask
        setup_ray<SPEC>(P, r);
        if (COUNT && st == ST_TRACING) n_sph += P.n_big;
        // Grid kernels always have a grid to walk: a compile-time fact instead of the launch test
        // (a loop-invariant lane mask the compiler spilled and reloaded every segment). With the
        // two changes beside it (the inert big-sphere records, the regate flag as a scalar select):
        // config 3 -1.2 %, DESIGN.md §5.
        if constexpr (LAYOUT == LAYOUT_GRID || LAYOUT == LAYOUT_GRID_L2 || LAYOUT == LAYOUT_GRID_COOP ||
                      LAYOUT == LAYOUT_GRID_CQ)
            r.walk = true;
        STAMP(2);
        if constexpr (LAYOUT == LAYOUT_GRID_COOP) {   // every lane of the wave takes part (tracing or not)
            grid_walk_coop<COUNT>(P, reinterpret_cast<const uint32_t*>(nodes4), leaf4, leaf_ids, r, st == ST_TRACING,
                                  n_box, n_sph);
        } else {
            if (st == ST_TRACING) walk<COUNT, LAYOUT, FLAT>(P, nodes4, leaf4, leaf_ids, r, n_box, n_sph, n_empty);
        }
        // the AABB gate of the winner only (winner_gated); the rare lanes whose winner fails it
        // get the contract's answer by a wave-cooperative gated brute force. The winner's shading
        // records are loaded with the gate's (one round trip to L2 per segment, not two).
        HitRec hr{};
        float rad = 0.0f;
        if (st == ST_TRACING && r.bi != 0xffffffffu) {
            if constexpr (REC) hr = load_hit_rec(r.bi);
            else hr = load_hit(geom4, mat4, r.bi);
            rad = REC ? hr.g.w : P.radius[r.bi];
        }
        // (the test-only flag replaces the ballot by a scalar select: folded into the per-lane
        // predicate it became a loop-invariant 64-bit lane mask the compiler spilled and reloaded)
        unsigned long long regate = __ballot(
            st == ST_TRACING && r.bi != 0xffffffffu && !aabb_hit(hr.g.x, hr.g.y, hr.g.z, rad, r.o, r.inv));
        if (P.force_regate) regate = __ballot(st == ST_TRACING);
        if (__builtin_expect(regate != 0ull, 0)) {
            regate_brute<COUNT>(P, reinterpret_cast<const float4*>(P.geom), lane, regate, r);
            if (((regate >> lane) & 1ull) && r.bi != 0xffffffffu) {
                if constexpr (REC) hr = load_hit_rec(r.bi);
                else hr = load_hit(geom4, mat4, r.bi);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (COUNT && st == ST_TRACING) {   // walk-length histogram (diagnostic, COUNT builds only)
            const uint32_t len = min(n_box - box0, 63u);
            atomicAdd(&P.counters->walk_hist[r.bi != 0xffffffffu ? 1 : 0][len], 1ull);
        }
        if (COUNT) {   // wave iterations of this walk = the longest lane walk
            uint32_t m = n_box - box0;
            for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off));
            if (lane == 0) wave_iters += m;
        }
        STAMP(3);
        bool fresh = false;   // a sample started inside shade()
        if (st == ST_TRACING) {
            ps.segs++;
            if (!shade_rec<MODE, LSUM, SPEC>(P, cam, hr, ps, r.bi, r.best, r.o, r.d, fresh)) {
                // The unit's last sample ended: finish it here, and the lane asks for a unit at
                // the top of the next iteration.
                finish_unit<MODE, LSUM>(P, ps);
                record_tile_cost<MODE>(P, ps);
                st = ST_NEED_UNIT;
            }
        }
        smp_w += __popcll(__ballot(fresh));
    }
    STAMP_FLUSH;
    if (lane == 0) {
        atomicAdd(&P.counters->segments, (unsigned long long)seg_w);
        atomicAdd(&P.counters->samples, (unsigned long long)smp_w);
        atomicMax(&P.counters->t_last, __builtin_amdgcn_s_memrealtime());
    }
    if (COUNT) {
        atomicAdd(&P.counters->box_tests, (unsigned long long)n_box);
        atomicAdd(&P.counters->sphere_tests, (unsigned long long)n_sph);
        if (n_empty) atomicAdd(&P.counters->cells_empty, (unsigned long long)n_empty);
        if (lane == 0) atomicAdd(&P.counters->wave_iters, wave_iters);
    }
    UTIL_FLUSH;
}

// LBVH kernel, tree in global memory (A/B reference: every node and leaf from L2).
template <bool COUNT, int MODE, int TAB = 0>
__global__ __launch_bounds__(kTraceBlock, RT_TRACE_WAVES_PER_SIMD) void rt_trace_global_kernel(const rt::TraceParams P) {
    UTIL_INIT;
    PLACEMENT_RECORD(P);
    stage_walk_params(P, threadIdx.x);
    stage_rows(P, threadIdx.x, kTraceBlock);
    __syncthreads();
    lbvh_loop<COUNT, LAYOUT_GLOBAL, MODE, false, false, TAB>(P, reinterpret_cast<const float4*>(P.nodes),
                                          reinterpret_cast<const float4*>(P.leaf_geom), P.leaf_ids,
                                          reinterpret_cast<const float4*>(P.geom),
                                          reinterpret_cast<const float4*>(P.mat));
}

// LBVH kernel with the whole tree staged in LDS, once per persistent block (one 1024-thread block
// per CU). Staged nodes use the AB layout (node_hit); NOCT = 8 stages one copy per ray direction
// octant, each in its own near-child-first order when the host provides one (nodes_oct). LDS:
// [nodes | leaf spheres | leaf ids]. The geometry + material records read by
// shading stay in HBM: one random record per hit is an L2 hit (staging them in LDS measured the
// same), and the LDS they would take fits bigger trees as octant copies.
template <bool COUNT, uint32_t NOCT, int MODE, int TAB = 0>
__global__ __launch_bounds__(kTraceBlock, RT_TRACE_WAVES_PER_SIMD) void rt_trace_lds_kernel(const rt::TraceParams P) {
    UTIL_INIT;
    PLACEMENT_RECORD(P);
    extern __shared__ float4 lds[];
    typedef const __attribute__((address_space(3))) float4* LdsF4;
    const uint32_t lbase = uint32_t(reinterpret_cast<uintptr_t>((LdsF4)lds));   // LDS address of lds[0]
    const uint32_t n_node4 = 2u * NOCT * P.n_nodes, n_leaf4 = P.n_leaf, n_id4 = (P.n_leaf + 3u) / 4u;
    constexpr uint32_t kNodeBytes = 32u;
    const float4* nodes4 = reinterpret_cast<const float4*>(P.nodes);
    for (uint32_t oi = threadIdx.x; oi < NOCT * P.n_nodes; oi += kTraceBlock) {
        const uint32_t o = oi / P.n_nodes, i = oi - o * P.n_nodes;   // copy o, node i
        // BvhNode: lo.xyz escape, hi.xyz leaf.
        const float4* src = (NOCT == 8 && P.nodes_oct)
                                ? reinterpret_cast<const float4*>(P.nodes_oct + size_t(o) * P.n_nodes)
                                : nodes4;
        const float4 lo = src[2 * i], hi = src[2 * i + 1];
        // Links (walk, AB layout): LDS address of the target node in this copy, END = ~0; a hit
        // leaf yields 0x80000000 | escape node << 12 | leaf index << 2 | (count - 1), escape node
        // = 0x7ffff for END. (Trees staged in LDS have < 2^14 nodes and < 1024 leaves of <= 4
        // slots, checked by the host.)
        const uint32_t esc = __float_as_uint(lo.w), fc = __float_as_uint(hi.w);
        const bool nx = NOCT == 8 && (o & 1u), ny = NOCT == 8 && (o & 2u), nz = NOCT == 8 && (o & 4u);
        const uint32_t cb = o * P.n_nodes;   // first node of copy o
        const uint32_t miss = esc == END ? END : lbase + (cb + esc) * kNodeBytes;
        // (kept as separate statements: one combined expression crashed the ROCm 7.2 instruction
        // selector)
        const uint32_t escf = esc == END ? 0x7ffffu : cb + esc;
        const uint32_t leafw = 0x80000000u + (escf << 12) + ((fc >> 6) << 2) + ((fc - 1u) & 3u);
        const uint32_t hit = fc ? leafw : lbase + (cb + i + 1u) * kNodeBytes;
        const size_t b = size_t(cb + i) * 2u, bb = b + 1u;
        lds[b] = make_float4(nx ? hi.x : lo.x, ny ? hi.y : lo.y, nx ? lo.x : hi.x, ny ? lo.y : hi.y);
        lds[bb] = make_float4(nz ? hi.z : lo.z, nz ? lo.z : hi.z, __uint_as_float(miss), __uint_as_float(hit));
    }
    const float4* leaf4 = reinterpret_cast<const float4*>(P.leaf_geom);
    for (uint32_t i = threadIdx.x; i < n_leaf4; i += kTraceBlock) lds[n_node4 + i] = leaf4[i];
    const uint4* ids4 = reinterpret_cast<const uint4*>(P.leaf_ids);
    for (uint32_t i = threadIdx.x; i < n_id4; i += kTraceBlock) {
        const uint4 v = ids4[i];
        lds[n_node4 + n_leaf4 + i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y),
                                                 __uint_as_float(v.z), __uint_as_float(v.w));
    }
    const float4* geom4 = reinterpret_cast<const float4*>(P.geom);
    const float4* mat4 = reinterpret_cast<const float4*>(P.mat);
    stage_walk_params(P, threadIdx.x);
    stage_rows(P, threadIdx.x, kTraceBlock);
    __syncthreads();
    lbvh_loop<COUNT, NOCT == 8 ? LAYOUT_OCT : LAYOUT_LDS1, MODE, false, false, TAB>(
        P, lds, lds + n_node4, reinterpret_cast<const uint32_t*>(lds + n_node4 + n_leaf4), geom4, mat4);
}

// Grid kernel (ACCEL_GRID): the grid's cell offsets and references staged in LDS once per
// persistent block: [references (float4) | reference ids | cell offsets] in dynamic LDS, and with
// REC the shading records in the static table s_rec.
// FLAT: the grid is one cell thick in y, as every grid of a scene whose small spheres lie in one
// layer is (configs 3 and 5): the DDA steps x and z only (grid_walk; launch_trace picks it).
template <bool COUNT, int MODE, bool IN_LDS, bool COOP = false, bool REC = false, bool CQ = false, bool FLAT = false,
          int TAB = 0>
__global__ __launch_bounds__(kTraceBlock, RT_TRACE_WAVES_PER_SIMD) void rt_trace_grid_kernel(const rt::TraceParams P) {
    UTIL_INIT;
    PLACEMENT_RECORD(P);
    extern __shared__ float4 lds[];
    if (!IN_LDS) {   // grids too big for LDS: offsets and references from L2 / HBM
        stage_walk_params(P, threadIdx.x);
        stage_rows(P, threadIdx.x, kTraceBlock);
        __syncthreads();
        lbvh_loop<COUNT, COOP ? LAYOUT_GRID_COOP : LAYOUT_GRID_L2, MODE, false, FLAT, TAB>(P, reinterpret_cast<const float4*>(P.cell_start),
                                            reinterpret_cast<const float4*>(P.grid_rec), P.grid_ids,
                                            reinterpret_cast<const float4*>(P.geom),
                                            reinterpret_cast<const float4*>(P.mat));
        return;
    }
    const uint32_t nr = P.grid.n_refs, nc1 = P.grid.n_cells + 1u;
    const uint32_t n_id4 = (nr + 3u) / 4u;
    const float4* rec = reinterpret_cast<const float4*>(P.grid_rec);
    for (uint32_t i = threadIdx.x; i < nr; i += kTraceBlock) lds[i] = rec[i];
    uint32_t* ids = reinterpret_cast<uint32_t*>(lds + nr);
    for (uint32_t i = threadIdx.x; i < nr; i += kTraceBlock) ids[i] = P.grid_ids[i];
    uint32_t* cst = reinterpret_cast<uint32_t*>(lds + nr + n_id4);
    for (uint32_t i = threadIdx.x; i < nc1; i += kTraceBlock) cst[i] = P.cell_start[i];
    stage_walk_params(P, threadIdx.x);
    stage_rows(P, threadIdx.x, kTraceBlock);
    if (REC) {   // the winner's gate and shading records in LDS too: {cx, cy, cz, r} + 2 x MatRec float4
        const float4* mat4 = reinterpret_cast<const float4*>(P.mat);
        const uint32_t n = min(P.n_spheres, rt::kRecStatic);   // the host picks REC only within the table
        for (uint32_t i = threadIdx.x; i < n; i += kTraceBlock) {
            const rt::GeomRec g = P.geom[i];
            s_rec[3 * i] = make_float4(g.cx, g.cy, g.cz, P.radius[i]);
            s_rec[3 * i + 1] = mat4[2 * i];
            s_rec[3 * i + 2] = mat4[2 * i + 1];
        }
        __syncthreads();
        lbvh_loop<COUNT, CQ ? LAYOUT_GRID_CQ : LAYOUT_GRID, MODE, true, FLAT, TAB>(P, reinterpret_cast<const float4*>(cst), lds,
                                                                              ids, s_rec, s_rec);   // (load_hit_rec)
        return;
    }
    __syncthreads();
    lbvh_loop<COUNT, COOP ? LAYOUT_GRID_COOP : CQ ? LAYOUT_GRID_CQ : LAYOUT_GRID, MODE, false, FLAT, TAB>(P, reinterpret_cast<const float4*>(cst), lds, ids,
                                        reinterpret_cast<const float4*>(P.geom),
                                        reinterpret_cast<const float4*>(P.mat));
}

// Camera-batch form of the LDS grid kernel (rt_trace_batch.h): HASH launches with the uniform
// hand-out whose plan proved pinhole_lf and a two-block LDS budget (launch_trace_batch's callers). The
// grid is staged as in rt_trace_grid_kernel; the winner's gate records and the camera-origin terms
// are staged in the form's own static LDS (s_gate, s_cam_tab), the shading records come from L2
// (the static table s_rec does not fit beside the path queue). A kernel of its own, so that every
// other kernel keeps its name and its code.
template <bool FLAT>
__global__ __launch_bounds__(kTraceBlock, RT_TRACE_WAVES_PER_SIMD) void rt_trace_grid_batch_kernel(const rt::TraceParams P) {
    UTIL_INIT;
    PLACEMENT_RECORD(P);
    extern __shared__ float4 lds[];
    const uint32_t nr = P.grid.n_refs, nc1 = P.grid.n_cells + 1u;
    const uint32_t n_id4 = (nr + 3u) / 4u;
    const float4* rec = reinterpret_cast<const float4*>(P.grid_rec);
    for (uint32_t i = threadIdx.x; i < nr; i += kTraceBlock) lds[i] = rec[i];
    uint32_t* ids = reinterpret_cast<uint32_t*>(lds + nr);
    for (uint32_t i = threadIdx.x; i < nr; i += kTraceBlock) ids[i] = P.grid_ids[i];
    uint32_t* cst = reinterpret_cast<uint32_t*>(lds + nr + n_id4);
    for (uint32_t i = threadIdx.x; i < nc1; i += kTraceBlock) cst[i] = P.cell_start[i];
    stage_walk_params(P, threadIdx.x);
    stage_rows(P, threadIdx.x, kTraceBlock);
    stage_gate(P, threadIdx.x, kTraceBlock);
    stage_camera_terms(P, threadIdx.x);
    __syncthreads();
    batch_loop<FLAT>(P, reinterpret_cast<const float4*>(cst), lds, ids, reinterpret_cast<const float4*>(P.geom),
                     reinterpret_cast<const float4*>(P.mat));
    UTIL_FLUSH;
}

// LBVH kernel for trees too big for LDS: the treelet (rt_build.hip build_treelet) is staged in LDS
// with its rank links turned into LDS addresses; leaves, subtrees below the cut, geometry and
// materials stay in HBM/L2.
template <bool COUNT, int MODE, int TAB = 0>
__global__ __launch_bounds__(kTraceBlock, RT_TRACE_WAVES_PER_SIMD) void rt_trace_top_kernel(const rt::TraceParams P) {
    UTIL_INIT;
    PLACEMENT_RECORD(P);
    extern __shared__ float4 lds[];
    typedef const __attribute__((address_space(3))) float4* LdsF4;
    const uint32_t lbase = uint32_t(reinterpret_cast<uintptr_t>((LdsF4)lds));
    const uint32_t n_top = min(*P.treelet_count, rt::kTreeletCap);
    for (uint32_t i = threadIdx.x; i < n_top; i += kTraceBlock) {
        const float4* tl = reinterpret_cast<const float4*>(P.treelet);
        const float4 A = tl[2 * i], B = tl[2 * i + 1];
        const uint32_t miss = __float_as_uint(B.z), hit = __float_as_uint(B.w);
        lds[2 * i] = A;
        lds[2 * i + 1] = make_float4(B.x, B.y, __uint_as_float(miss == END ? END : lbase + miss * 32u),
                                     __uint_as_float(int32_t(hit) >= 0 ? lbase + hit * 32u : hit));
    }
    stage_walk_params(P, threadIdx.x);
    stage_rows(P, threadIdx.x, kTraceBlock);
    __syncthreads();
    lbvh_loop<COUNT, LAYOUT_TOP, MODE, false, false, TAB>(P, lds, reinterpret_cast<const float4*>(P.leaf_geom), P.leaf_ids,
                                       reinterpret_cast<const float4*>(P.geom),
                                       reinterpret_cast<const float4*>(P.mat));
}

}  // namespace

// ---- host-callable launchers (rt_launchers.h) -----------------------------------------------
namespace rt {

// TAB: the table form of the hand-out (TraceParams::block_tab), HASH launches only: 1 a table whose
// size is in the kernel argument, 2 one whose size is a device record (TraceParams::tab_size). Two
// instantiations, not a branch on P.tab_size: the host-table kernels keep their source (DESIGN.md
// §3.1.2 measured the one-instantiation form 0.4-1 % slower on them).
// The one table from a launch's form to its kernel. COUNT is a template argument so that a mode
// instantiates only the instrumented kernels it has (pick_mode).
template <int MODE, int TAB, bool COUNT>
static const void* pick_form(uint32_t accel, bool flat) {
#define RT_FN(...) reinterpret_cast<const void*>(__VA_ARGS__)
#define RT_GRID(IN_LDS, COOP, REC, CQ, FLAT) RT_FN(rt_trace_grid_kernel<COUNT, MODE, IN_LDS, COOP, REC, CQ, FLAT, TAB>)
    if constexpr (!COUNT) {   // the grid walks of one-layer grids (instrumented builds count the same cells
                              // with the general form: they have no one-layer kernels)
        if (flat) {
            switch (accel) {
                case ACCEL_GRID: return RT_GRID(true, false, false, false, true);
                case ACCEL_GRID_REC: return RT_GRID(true, false, true, false, true);
                case ACCEL_GRID_GLOBAL: return RT_GRID(false, false, false, false, true);
                default: break;
            }
        }
    }
    switch (accel) {
        case ACCEL_BRUTE: return RT_FN(rt_trace_brute_kernel<COUNT, MODE, TAB>);
        case ACCEL_LBVH_LDS: return RT_FN(rt_trace_lds_kernel<COUNT, 1u, MODE, TAB>);
        case ACCEL_LBVH_OCT: return RT_FN(rt_trace_lds_kernel<COUNT, 8u, MODE, TAB>);
        case ACCEL_LBVH_TOP: return RT_FN(rt_trace_top_kernel<COUNT, MODE, TAB>);
        case ACCEL_GRID: return RT_GRID(true, false, false, false, false);
        case ACCEL_GRID_COOP: return RT_GRID(true, true, false, false, false);
        case ACCEL_GRID_REC: return RT_GRID(true, false, true, false, false);
        case ACCEL_GRID_CQ: return RT_GRID(true, false, false, true, false);
        case ACCEL_GRID_REC_CQ: return RT_GRID(true, false, true, true, false);
        case ACCEL_GRID_GLOBAL_COOP: return RT_GRID(false, true, false, false, false);
        case ACCEL_GRID_GLOBAL: return RT_GRID(false, false, false, false, false);
        default: return RT_FN(rt_trace_global_kernel<COUNT, MODE, TAB>);
    }
#undef RT_GRID
#undef RT_FN
}

// PROBE launches (rt_debug_closest_hits) and FEATURES launches (rt_render_features_device) are never
// instrumented: those modes have no COUNT kernels.
template <int MODE, int TAB>
static const void* pick_mode(uint32_t accel, bool count, bool flat) {
    if constexpr (MODE != MODE_PROBE && MODE != MODE_FEATURES) {
        if (count) return pick_form<MODE, TAB, true>(accel, flat);
    }
    return pick_form<MODE, TAB, false>(accel, flat);
}

static const void* pick(uint32_t accel, bool count, int mode, bool flat, int tab = 0) {
    if (mode == MODE_PROBE) return pick_mode<MODE_PROBE, 0>(accel, false, flat);
    if (mode == MODE_FEATURES) return pick_mode<MODE_FEATURES, 0>(accel, false, flat);
    if (mode != MODE_HASH) return pick_mode<MODE_STREAM, 0>(accel, count, flat);
    if (tab == 2) return pick_mode<MODE_HASH, 2>(accel, count, flat);
    return tab ? pick_mode<MODE_HASH, 1>(accel, count, flat) : pick_mode<MODE_HASH, 0>(accel, count, flat);
}

bool flat_grid_form(const TraceParams& P, uint32_t accel, bool count) {
    if (accel == ACCEL_GRID_GLOBAL && !(P.n_big <= 4u && P.pinhole_lf)) return false;   // (lbvh_loop SPEC)
    return !count && P.cell_start != nullptr && P.grid.n[1] == 1u &&
           (accel == ACCEL_GRID || accel == ACCEL_GRID_REC || accel == ACCEL_GRID_GLOBAL);
}

uint32_t block_size(uint32_t accel) { return accel == ACCEL_BRUTE ? kBruteBlock : kTraceBlock; }

hipError_t launch_trace(const TraceParams& P, uint32_t accel, bool count, int mode, int grid, size_t lds_bytes,
                        hipStream_t st) {
    void* args[] = {const_cast<TraceParams*>(&P)};
    // (the table form's occupancy is its uniform twin's: the same launch bounds and LDS; a probe
    // launch is planned as the STREAM launch of its band, and so is a features launch: one unit per
    // pixel holding all its samples)
    if (P.probe_rays) mode = MODE_PROBE;
    if (P.feat0) mode = MODE_FEATURES;
    return hipLaunchKernel(pick(accel, count, mode, flat_grid_form(P, accel, count), P.block_tab ? (P.tab_size ? 2 : 1) : 0), dim3(grid),
                           dim3(block_size(accel)),
                           args, lds_bytes, st);
}

hipError_t trace_occupancy(uint32_t accel, bool count, int mode, bool flat, size_t lds_bytes, int* blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, pick(accel, count, mode, flat),
                                                        block_size(accel), lds_bytes);
}

// The camera-batch form (rt_trace_batch.h): the one-layer LDS grid walk of a HASH launch with the
// uniform hand-out; the plan decides (rt_launch.h camera_batches), rt_render_device launches.
hipError_t launch_trace_batch(const TraceParams& P, int grid, size_t lds_bytes, hipStream_t st) {
    void* args[] = {const_cast<TraceParams*>(&P)};
    return hipLaunchKernel(reinterpret_cast<const void*>(rt_trace_grid_batch_kernel<true>), dim3(grid), dim3(kTraceBlock),
                           args, lds_bytes, st);
}

hipError_t trace_batch_occupancy(size_t lds_bytes, int* blocks_per_cu, size_t* static_lds) {
    hipFuncAttributes a;
    if (hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(rt_trace_grid_batch_kernel<true>)); e != hipSuccess)
        return e;
    *static_lds = a.sharedSizeBytes;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks_per_cu, reinterpret_cast<const void*>(rt_trace_grid_batch_kernel<true>), kTraceBlock, lds_bytes);
}

}  // namespace rt
