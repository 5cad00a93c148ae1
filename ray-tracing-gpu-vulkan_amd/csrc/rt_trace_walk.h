// rt_trace_walk.h — the closest-hit search of one segment (device only): the per-ray setup with
// the exhaustive big spheres, the node slab test and the stackless LBVH walks (tree in L2, tree in
// LDS, LDS treelet over L2 subtrees), the winner's AABB gate with its gated brute-force fallback,
// and walk(), which dispatches a walk form (the one-ray grid walks are rt_trace_grid.h's and
// rt_trace_grid_cq.h's). Stands in for the driver traversal of the reference (src/vulkan.h:395-554)
// with shaders/shader.rint:44-60 as its intersection test and src/ray_trace.cpp:586-596 as its gate.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"
#include "rt_trace_grid.h"
#include "rt_trace_grid_cq.h"
#include "rt_trace_prims.h"

using namespace rtd;

namespace {

// ---------------------------------------------------------------------------------------------
// LBVH traversal state and walks.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t END = 0xffffffffu;

// Walk forms (template LAYOUT): GLOBAL = escape-link BvhNode pairs from L2 (A/B reference of TOP),
// LDS1 = one node copy in LDS (AB layout), OCT = 8 octant-specialised copies in LDS, TOP = LDS
// treelet over L2 subtrees.
enum : int { LAYOUT_GLOBAL = 0, LAYOUT_LDS1 = 1, LAYOUT_OCT = 2, LAYOUT_TOP = 3, LAYOUT_GRID = 4, LAYOUT_GRID_L2 = 5,
             LAYOUT_GRID_COOP = 6, LAYOUT_GRID_CQ = 7 };

// Node slab test: one fma per plane, t = fma(plane, inv, -o * inv) (a sub-then-mul form is exact
// in the gate's own arithmetic but costs twice the issue cycles: packed f32 ops take 4 cycles on
// gfx950). Node boxes are padded at build time by 12u x (scene + camera radius),
// which covers the rounding of this form against the spheres' AABB gates.
// A zero (or denormal) direction component makes 1/d infinite; the fma form would then produce
// inf - inf = NaN for a plane on the far side of the origin and cull a box the ray runs inside, so
// the node reciprocal is clamped to +-2^100: the slab then spans (-huge, +huge) exactly when the
// origin lies inside the padded slab, which is what the gate's (plane - o) * inf gives.
// The same holds for a reciprocal that is finite but beyond 2^100 (a direction component below
// 2^-100, e.g. a denormal one): o * inv overflows to inf once |o| |inv| reaches 2^128, and the
// slab becomes (-inf, NaN), a cull of a box the ray runs inside (found by the closest-hit probe:
// tests/test_gpu_closest_hit.py test_denormal_direction_regression). Along such an axis the ray
// moves less than tmax 2^-100, far less than the boxes' padding, so it is inside the padded slab for
// its whole length or never: every |inv| > 2^100 is clamped, not the infinite one alone.
// Node layout "AB" (LDS): A = (x0, y0, x1, y1), B = (z0, z1, miss link, hit link). OCT: the node
// copy is specialised to the ray's direction octant, (x0, y0, z0) are the near planes and (x1, y1,
// z1) the far ones, so no per-axis min/max is needed.
struct RayBox { V3 inv, oi; };

__device__ __forceinline__ float node_inv(float inv) {
    return __builtin_fabsf(inv) > 0x1p100f ? __builtin_copysignf(0x1p100f, inv) : inv;
}
__device__ __forceinline__ RayBox ray_box(const V3 o, const V3 inv) {
    const V3 n = v3(node_inv(inv.x), node_inv(inv.y), node_inv(inv.z));
    return RayBox{n, v3(o.x * n.x, o.y * n.y, o.z * n.z)};
}

template <uint32_t NOCT>   // node copies per ray direction class: 1 (none) or 8 (octants)
__device__ __forceinline__ bool node_hit(const float4 A, const float4 B, const RayBox& q, float limit) {
    const float tx0 = __builtin_fmaf(A.x, q.inv.x, -q.oi.x), ty0 = __builtin_fmaf(A.y, q.inv.y, -q.oi.y);
    const float tx1 = __builtin_fmaf(A.z, q.inv.x, -q.oi.x), ty1 = __builtin_fmaf(A.w, q.inv.y, -q.oi.y);
    const float tz0 = __builtin_fmaf(B.x, q.inv.z, -q.oi.z), tz1 = __builtin_fmaf(B.y, q.inv.z, -q.oi.z);
    float tn, tf;
    if (NOCT == 8) {
        tn = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, T_MIN));
        tf = fminf(fminf(tx1, ty1), tz1);
    } else {
        tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), T_MIN));
        tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
    }
    // == tn <= min(tf, limit): limit is never NaN, so splitting the min into a second compare
    // gives the same answer without re-canonicalising the loop-invariant limit every visit.
    return tn <= tf && tn <= limit;
}

// 16-B load from an LDS address held in a register (ds_read_b128 addr, no base add).
__device__ __forceinline__ float4 lds_f4(uint32_t addr) {
    const f4v v = *(const __attribute__((address_space(3))) f4v*)(uintptr_t)addr;
    return make_float4(v.x, v.y, v.z, v.w);
}

// Octant of a direction: bit k set when component k is negative (sign bit, so -0 -> 1/d = -inf
// counts as negative, matching the copy whose near plane is the box's high side).
__device__ __forceinline__ uint32_t octant(const V3 d) {
    return (__float_as_uint(d.x) >> 31) | ((__float_as_uint(d.y) >> 31) << 1) | ((__float_as_uint(d.z) >> 31) << 2);
}

// Four big spheres (records sb, ids ib; SGPR operands): the discriminants, then a candidate tail
// per sphere that any lane needs (wave-uniform record: no reload, no per-lane select).
__device__ __forceinline__ void big_group(Ray& r, const float (&sb)[16], const uint32_t (&ib)[4]) {
    float bk[4], Dk[4];
    uint32_t cand = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float rr = sb[4 * k + 3] * sb[4 * k + 3];
        const float ocx = r.o.x - sb[4 * k], ocy = r.o.y - sb[4 * k + 1], ocz = r.o.z - sb[4 * k + 2];
        bk[k] = __builtin_fmaf(ocz, r.d.z, __builtin_fmaf(ocy, r.d.y, ocx * r.d.x));
        const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
        Dk[k] = __builtin_fmaf(bk[k], bk[k], -(r.a * c));
        cand |= (Dk[k] >= 0.0f && !behind(bk[k], c) ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((cand >> k) & 1u) {
            const float sq = sqrt_cr(Dk[k]);
            float t = (-bk[k] - sq) * r.ia;
            if (!(t >= T_MIN)) t = (-bk[k] + sq) * r.ia;   // report t1 if t1 >= tmin, else t2
            const uint32_t id = ib[k];
            if ((t >= T_MIN) & (t <= r.best) & ((t < r.best) | (id < r.bi))) {
                r.best = t;
                r.bi = id;
            }
        }
    }
}

// big_group for the camera-batch kernel's generation batches: the rays start at cam.lf, so oc and c
// of the four spheres come from s_cam_tab (stage_camera_terms: big_group's own expressions on lf,
// once per block) instead of seven VALU per sphere and lane; b, D and the candidate tails are
// big_group's. A lane whose origin is NaN (lens sample (0, 0)) needs no special case: its d is NaN,
// so b and D are NaN with either oc, D >= 0 is false and the lane has no candidate, as now.
__device__ __forceinline__ void big_group_camera(Ray& r, const uint32_t (&ib)[4]) {
    float bk[4], Dk[4];
    uint32_t cand = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 q = s_cam_tab[k];   // {oc.x, oc.y, oc.z, c}: one wave-uniform ds_read_b128
        bk[k] = __builtin_fmaf(q.z, r.d.z, __builtin_fmaf(q.y, r.d.y, q.x * r.d.x));
        Dk[k] = __builtin_fmaf(bk[k], bk[k], -(r.a * q.w));
        cand |= (Dk[k] >= 0.0f && !behind(bk[k], q.w) ? 1u : 0u) << k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((cand >> k) & 1u) {
            const float sq = sqrt_cr(Dk[k]);
            float t = (-bk[k] - sq) * r.ia;
            if (!(t >= T_MIN)) t = (-bk[k] + sq) * r.ia;   // report t1 if t1 >= tmin, else t2
            const uint32_t id = ib[k];
            if ((t >= T_MIN) & (t <= r.best) & ((t < r.best) | (id < r.bi))) {
                r.best = t;
                r.bi = id;
            }
        }
    }
}

// New segment: hoisted per-ray terms and the exhaustive big spheres.
// CAMERA: a generation batch of the camera-batch kernel (big_group_camera).
template <bool FAST = false, bool CAMERA = false>   // FAST: at most 4 big spheres (the one-layer L2 grid kernel, lbvh_loop SPEC)
__device__ __forceinline__ void setup_ray(const rt::TraceParams& P, Ray& r) {
    // records and ids through the scalar cache (TraceParams::big_tab, SGPR operands, no LDS round
    // trip: config 3 -1.6 %, reference stream -1.7 %, config 5 -2.2 % against an LDS table); the
    // four discriminants stay in registers for the candidate passes, which run per sphere with a
    // wave-uniform record (no reload, no per-lane record select)
    typedef const __attribute__((address_space(4))) float* ConstF;
    typedef const __attribute__((address_space(4))) uint32_t* ConstU;
    const ConstF g = (ConstF)(P.big_tab);
    const ConstU gid = (ConstU)(P.big_tab + 4u * rt::kBigMax);
    // the first four records and ids are requested before the reciprocals, so the scalar loads'
    // latency runs under them (the table always holds kBigMax entries: reading the first four is
    // safe whatever n_big); the ids come with the records, not one dependent load per candidate
    float sb0[16];
    uint32_t ib0[4];
    if constexpr (!CAMERA) {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) sb0[k] = g[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) ib0[k] = gid[k];
    r.a = dot(r.d, r.d);
    r.ia = rcp_cr(r.a);
    r.inv = v3(rcp_cr(r.d.x), rcp_cr(r.d.y), rcp_cr(r.d.z));
    // closest so far: none, with t <= tMax (shader.rint:32-39 reports t <= tMax). The walks accept
    // (t <= best, lowest id on ties), so best = 10000 exactly accepts a report at tMax and nothing
    // beyond it, and the (t bits, id) keys of the cooperative walk order the same way.
    r.best = 10000.0f;
    r.bi = 0xffffffffu;
    if constexpr (CAMERA) big_group_camera(r, ib0);
    else big_group(r, sb0, ib0);   // (without big spheres the table holds four inert records: no test)
    for (uint32_t k0 = 4; !FAST && k0 < P.n_big; k0 += 4) {
        float sb[16];
        uint32_t ib[4];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) sb[k] = g[k0 * 4u + k];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) ib[k] = gid[k0 + k];
        big_group(r, sb, ib);
    }
    r.limit = cull_limit(P, r.best);
    r.walk = P.nodes != nullptr || P.cell_start != nullptr;
}

// Leaf of 4 slots (dummy-padded), loads issued together; the candidate loop reloads a record
// (test4 RELOAD) from LDS (LDS_LEAF: staged leaves) or from L2. Reloading from L2 in the treelet
// kernel measured 6.5 % faster (config 5 at 20 spp: 39.6 -> 37.0 ms; its spills 34 -> 0).
template <bool COUNT, bool LDS_LEAF>
__device__ __forceinline__ void leaf_test(const rt::TraceParams& P, const float4* __restrict__ leaf4,
                                          const uint32_t* __restrict__ leaf_ids, uint32_t first,
                                          uint32_t count, Ray& r, uint32_t& n_sph) {
    const float4 s0 = leaf4[first], s1 = leaf4[first + 1], s2 = leaf4[first + 2], s3 = leaf4[first + 3];
    test4(s0, s1, s2, s3, [&](uint32_t k) {
                       if (LDS_LEAF) return lds_reload(leaf4 + first + k);
                       const f4v v = *(const volatile __attribute__((address_space(1))) f4v*)(leaf4 + first + k);
                       return make_float4(v.x, v.y, v.z, v.w);
                   },
                    [&](uint32_t k) { return leaf_ids[first + k]; }, r.o, r.d, r.inv, r.a, r.ia, r.best,
                    r.bi, r.limit, P);
    if (COUNT) n_sph += count;
}

// Escape-link walk over BvhNode pairs in global memory (L2), nodes [gi, bound): escape in lo.w,
// leaf field (first << 4 | count, 0 = inner) in hi.w. While-while (Aila & Laine 2009): the cheap
// node loop runs until every lane has found a hit leaf or left the range; then the pending leaves
// are tested together.
template <bool COUNT>
__device__ __forceinline__ void walk_global_range(const rt::TraceParams& P, const float4* __restrict__ gnodes,
                                                  const float4* __restrict__ leaf4,
                                                  const uint32_t* __restrict__ leaf_ids, const RayBox& q,
                                                  uint32_t gi, uint32_t bound, Ray& r, uint32_t& n_box,
                                                  uint32_t& n_sph) {
    uint32_t pending = 0u;
    for (;;) {
        while (gi < bound && pending == 0u) {
            UTIL(11, true);
            const float4 n0 = gnodes[2 * gi];
            const float4 n1 = gnodes[2 * gi + 1];
            if (COUNT) n_box++;
            const bool h = node_hit<1>(make_float4(n0.x, n0.y, n1.x, n1.y), make_float4(n0.z, n1.z, 0.0f, 0.0f),
                                       q, r.limit);
            const uint32_t fc = __float_as_uint(n1.w);
            if (h && fc != 0u) pending = fc;
            gi = (h && fc == 0u) ? gi + 1u : __float_as_uint(n0.w);
        }
        if (pending == 0u) break;
        leaf_test<COUNT, false>(P, leaf4, leaf_ids, pending >> 4, pending & 15u, r, n_sph);
        pending = 0u;
    }
}

// The AABB gate of the segment's closest hit, tested once after the walk instead of for every
// candidate that improves the running best (in a divergent tail, each such pass cost the whole
// wave ~30 VALU). Exact: let R be the ungated winner (smallest (t, id) among the quadratic's
// reports the walk tested) and W the gated one (the contract's answer). If R passes the gate, R is
// in the gated set, so W <= R; the walk stops only once the next cell / node starts beyond
// limit(R) >= limit(W) (t_W <= t_R), and W's AABB entry lies before limit(W) (DESIGN.md §4.3
// (iii)), so W was tested and R <= W: R = W. If R fails the gate (a rounding corner: the quadratic
// reports a hit whose ray misses the box; ~1 segment in 7e7 on config 3), the segment's answer is
// recomputed by the contract's rule itself: gated brute force (regate_brute).
// REC: geom4 holds {cx, cy, cz, r} records staged in LDS (rt_trace_grid_kernel<..., REC>), else
// the HBM GeomRec array {cx, cy, cz, r^2} with the radii in P.radius.
template <bool REC>
__device__ __forceinline__ bool winner_gated(const rt::TraceParams& P, const float4* __restrict__ geom4, const Ray& r) {
    if (r.bi == 0xffffffffu) return true;
    const float4 g = geom4[r.bi];
    return aabb_hit(g.x, g.y, g.z, REC ? g.w : P.radius[r.bi], r.o, r.inv);
}

// Gated brute force for the lanes in `need` (wave-uniform), one ray at a time with the whole wave:
// lane k tests spheres k, k + 64, ... in index order (the contract's `t < best` rule keeps the
// lowest index on ties within a lane), then the wave takes the minimum of (t bits, id) — t >= tmin
// > 0, so float bits order like the values and the u64 minimum is the (t, lowest id) rule. 64x
// shorter than one lane walking the whole list (config 5: 99 860 spheres).
template <bool COUNT>
__device__ __forceinline__ void regate_brute(const rt::TraceParams& P, const float4* __restrict__ geom4, uint32_t lane,
                                          unsigned long long need, Ray& r) {
    if (COUNT && lane == 0) atomicAdd(&P.counters->util[30], (unsigned long long)__popcll(need));
    while (need) {
        const int L = __ffsll(need) - 1;
        need &= need - 1ull;
        const V3 o = v3(__shfl(r.o.x, L), __shfl(r.o.y, L), __shfl(r.o.z, L));
        const V3 d = v3(__shfl(r.d.x, L), __shfl(r.d.y, L), __shfl(r.d.z, L));
        const V3 inv = v3(__shfl(r.inv.x, L), __shfl(r.inv.y, L), __shfl(r.inv.z, L));
        const float a = __shfl(r.a, L), ia = __shfl(r.ia, L);
        float best = T_MAX_SUCC;
        uint32_t bi = 0xffffffffu;
        for (uint32_t i = lane; i < P.n_spheres; i += 64u) {
            const float4 s = geom4[i];
            test_sphere(s.x, s.y, s.z, s.w, P.radius, o, d, inv, a, ia, i, best, bi);
        }
        unsigned long long key = (uint64_t(__float_as_uint(best)) << 32) | bi;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long k2 = __shfl_xor(key, off);
            key = k2 < key ? k2 : key;
        }
        if (int(lane) == L) {
            r.best = __uint_as_float(uint32_t(key >> 32));
            r.bi = uint32_t(key);
        }
    }
}

// The whole walk of one segment. FLAT: the grid is one cell thick in y (grid_walk).
template <bool COUNT, int LAYOUT, bool FLAT = false, bool CAMERA = false>
__device__ __forceinline__ void walk(const rt::TraceParams& P, const float4* __restrict__ nodes4,
                                     const float4* __restrict__ leaf4, const uint32_t* __restrict__ leaf_ids,
                                     Ray& r, uint32_t& n_box, uint32_t& n_sph, uint32_t& n_empty) {
    if (LAYOUT == LAYOUT_GRID_CQ) {
        if (r.walk)
            grid_walk_cq<COUNT>(P, reinterpret_cast<const uint32_t*>(nodes4), leaf4, leaf_ids, r, n_box, n_sph, n_empty);
        return;
    }
    if (LAYOUT == LAYOUT_GRID || LAYOUT == LAYOUT_GRID_L2) {   // nodes4 = cell offsets, leaf4 / leaf_ids = references
        if (r.walk)
            grid_walk<COUNT, LAYOUT == LAYOUT_GRID_L2, FLAT, CAMERA>(P, reinterpret_cast<const uint32_t*>(nodes4), leaf4, leaf_ids,
                                                             r, n_box, n_sph, n_empty);
        return;
    }
    const RayBox q = ray_box(r.o, r.inv);
    typedef const __attribute__((address_space(3))) float4* LdsF4;
    if (LAYOUT == LAYOUT_GLOBAL) {
        walk_global_range<COUNT>(P, nodes4, leaf4, leaf_ids, q, r.walk ? 0u : P.n_nodes, P.n_nodes, r, n_box,
                                 n_sph);
    } else if (LAYOUT == LAYOUT_TOP) {
        // Treelet in LDS (top kTreeletDepth levels, AB layout with LDS-address links), the
        // subtrees below the cut and all leaf spheres from L2. A lane leaves the LDS loop at a hit
        // word — a leaf, or a subtree root at the cut — remembering the node's miss link, where it
        // continues afterwards (the escape of a leaf or of a whole subtree). In a balanced
        // 100 k-sphere tree the top 11 levels take ~72 % of the visits (scripts/visit_depths.py).
        const uint32_t nbase = uint32_t(reinterpret_cast<uintptr_t>((LdsF4)nodes4));
        const float4* gnodes = reinterpret_cast<const float4*>(P.nodes);
        uint32_t ni = r.walk ? nbase : END;
        for (;;) {
            uint32_t cont = END;
            while (int32_t(ni) >= 0) {
                UTIL(0, true);
                const float4 A = lds_f4(ni);
                const float4 B = lds_f4(ni + 16u);
                if (COUNT) n_box++;
                const bool hit = node_hit<1u>(A, B, q, r.limit);
                cont = __float_as_uint(B.z);
                ni = __float_as_uint(hit ? B.w : B.z);
            }
            const bool at = ni != END;
            if (!__ballot(at)) break;
            if (at) {
                UTIL(1, true);
                if (ni & 0x40000000u) {   // subtree of global node g (inner, its box was hit): [g + 1, escape(g))
                    const uint32_t g = ni & 0x3fffffffu;
                    const uint32_t eg = __float_as_uint(gnodes[2 * g].w);
                    walk_global_range<COUNT>(P, gnodes, leaf4, leaf_ids, q, g + 1u, eg == END ? P.n_nodes : eg, r,
                                             n_box, n_sph);
                } else {                  // leaf above the cut
                    const uint32_t fc = ni & 0x3fffffffu;
                    leaf_test<COUNT, false>(P, leaf4, leaf_ids, fc >> 4, fc & 15u, r, n_sph);
                }
                ni = cont;
            }
        }
    } else {
        // AB layout staged in LDS by the kernel: links are LDS addresses of the node, so a visit
        // needs no address arithmetic; B.z = link when the box is missed, B.w = link when it is
        // hit: the next node (inner node) or, bit 31 set, a leaf word (escape node | leaf index |
        // count - 1). END and leaf words are negative, so `continue` is one sign test. A lane
        // leaves the inner loop at a hit leaf holding its leaf word; the leaves are tested
        // together after the loop (while-while).
        const uint32_t nbase = uint32_t(reinterpret_cast<uintptr_t>((LdsF4)nodes4));   // LDS address of node 0
        constexpr uint32_t kNB = 32u, kBOff = 16u;
        uint32_t ni = r.walk ? nbase + (LAYOUT == LAYOUT_OCT ? octant(r.d) * P.n_nodes * kNB : 0u) : END;
        for (;;) {
            while (int32_t(ni) >= 0) {
                UTIL(0, true);
#ifdef RT_UTIL
                {   // node passes by active lanes: [12] <= 8 lanes, [13] <= 16, [14] <= 32 (+ lanes)
                    const uint32_t na = __popcll(__ballot(true));
                    if (na <= 8) UTIL(12, true);
                    if (na <= 16) UTIL(13, true);
                    if (na <= 32) UTIL(14, true);
                }
#endif
                const float4 A = lds_f4(ni);          // links are LDS addresses:
                const float4 B = lds_f4(ni + kBOff);  // no address arithmetic per visit
                if (COUNT) n_box++;
                const bool hit = node_hit<LAYOUT == LAYOUT_OCT ? 8u : 1u>(A, B, q, r.limit);
                ni = __float_as_uint(hit ? B.w : B.z);
            }
            const bool at_leaf = ni != END;
            if (!__ballot(at_leaf)) break;   // no lane stopped at a leaf: all walks done
            if (at_leaf) {
                UTIL(1, true);
                const uint32_t esc = (ni >> 12) & 0x7ffffu;
                leaf_test<COUNT, true>(P, leaf4, leaf_ids, ((ni >> 2) & 1023u) * 4u, (ni & 3u) + 1u, r, n_sph);
                ni = esc == 0x7ffffu ? END : nbase + esc * kNB;
            }
        }
    }
}

}  // namespace
