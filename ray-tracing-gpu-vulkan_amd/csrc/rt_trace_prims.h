// rt_trace_prims.h — the primitives every closest-hit search is made of (device only):
//   shaders/shader.rint:44-60   ray-sphere quadratic, t1-else-t2 report inside [tmin, tmax]
//                               (test_sphere; test4 / test1 for the walks' leaves and cells)
//   shaders/shader.rgen:26, :75 tMax and tMin
//   src/ray_trace.cpp:586-596   a sphere's AABB, the driver traversal's gate (aabb_hit)
// and, with no reference counterpart, the launch parameters the walk kernels stage in LDS, the grid
// walks' DDA step, the cull limit, the brute-force search through the scalar cache, and the
// segment's ray state (Ray).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"

using namespace rtd;

namespace {

constexpr float T_MIN = 0.001f;               // shader.rgen:75
constexpr float T_MAX_SUCC = 0x1.388002p+13f; // successor of 10000.0f (shader.rgen:26): a report
                                              // at exactly tMax is accepted, so compare with '<'.

// Driver traversal test for one sphere's AABB (src/ray_trace.cpp:586-596: center -/+ radius)
// over [T_MIN, T_MAX]; identical arithmetic to the oracle's aabb_hit.
__device__ __forceinline__ bool aabb_hit(float cx, float cy, float cz, float r, V3 o, V3 inv) {
    const float x0 = ((cx - r) - o.x) * inv.x, x1 = ((cx + r) - o.x) * inv.x;
    const float y0 = ((cy - r) - o.y) * inv.y, y1 = ((cy + r) - o.y) * inv.y;
    const float z0 = ((cz - r) - o.z) * inv.z, z1 = ((cz + r) - o.z) * inv.z;
    const float tnear = fmaxf(fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1)), T_MIN);
    const float tfar = fminf(fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)), 10000.0f);
    return tnear <= tfar;
}

// shader.rint:44-60 + the closest-hit rule for one sphere, spheres visited in index order: a
// candidate when the quadratic reports t (t1 if t1 >= tmin else t2) in [tmin, best) and the ray
// overlaps the sphere's AABB. The roots divide by a through its reciprocal ia = 1/a, computed
// once per segment (GLSL's division is 2.5-ulp, and AMD's Vulkan compilers emit
// x * rcp(y) for it too).
template <bool GATE = true>
__device__ __forceinline__ void test_sphere(float cx, float cy, float cz, float rr,
                                            const float* __restrict__ radius, V3 o, V3 d, V3 inv,
                                            float a, float ia, uint32_t id, float& best, uint32_t& bi) {
    const float ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const float b = __builtin_fmaf(ocz, d.z, __builtin_fmaf(ocy, d.y, ocx * d.x));
    const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
    const float D = __builtin_fmaf(b, b, -(a * c));
    if (D >= 0.0f) {
        const float sq = sqrt_cr(D);
        const float t1 = (-b - sq) * ia;
        const float t2 = (-b + sq) * ia;
        const float t = (t1 >= T_MIN) ? t1 : t2;
        if (t >= T_MIN && t < best && (!GATE || aabb_hit(cx, cy, cz, radius[id], o, inv))) {
            best = t;
            bi = id;
        }
    }
}

// Both roots behind the origin (outside the sphere, moving away from it): no report in [tmin,
// tmax], so the exact tail need not run. Exact: a >= 0 and c >= 0 give RN(a c) >= 0, so D =
// RN(b^2 - RN(a c)) <= RN(b^2) and sqrt_cr(D) <= sqrt_cr(RN(b^2)) = b (b >= 2^-60: b^2 is normal;
// an overflowing b^2 gives t2 = +inf, rejected by t <= best); then t1 and t2 are <= 0 < tmin.
// Typical cases: the sphere a bounce ray leaves (origin on it, c >= 0 after rounding) and spheres
// behind the ray whose line still crosses them.
__device__ __forceinline__ bool behind(float b, float c) { return b >= 0x1p-60f && c >= 0.0f; }

// 16-B reload of an LDS record inside a rarely run loop (volatile: not merged with the first
// load, so the record's registers are free in between).
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 lds_reload(const float4* p) {
    const f4v v = *(const volatile __attribute__((address_space(3))) f4v*)(p);
    return make_float4(v.x, v.y, v.z, v.w);
}

// Launch parameters that a lane selects per lane, staged in LDS by every walk kernel before its
// first barrier (stage_walk_params): per grid axis the DDA step's (cell size, origin, linear cell
// stride, cell count), one 16-B load per step, and the two absolute cull slacks. Read with a
// per-lane LDS address (lgkmcnt wait only) instead of the compiler's per-lane select of
// kernel-argument addresses and a global load, whose vmcnt(0) wait also waited for every store
// and atomic the wave had in flight; and the stride and count from the table instead of per-step
// integer multiplies and a scalar reload of a kernel argument that the SGPR budget evicted
// (config 3 -3.1 %, reference stream -2.9 %, config 5 -1.3 %).
__shared__ float4 s_walk_axis[3];   // (cs[k], gmin[k], stride[k], n[k]): stride and n as uint bits
__shared__ float2 s_walk_slack;     // (cull_near_abs, cull_abs)
// ... and the grid walk's entry parameters (the widened grid box, 1 / cell size, the last cell
// index per axis) from LDS as well, instead of kernel-argument reloads (an s_load and an
// lgkmcnt(0) wait, which also drains the wave's LDS reads, at every walk's entry) and spilled
// SGPRs (together with the early big-sphere loads of setup_ray: config 3 -2.2 %, reference
// stream -4.6 %, config 5 -1.5 %).
__shared__ float4 s_walk_entry[3];   // per axis: (lo_m, hi_m, inv_cs, n - 1 as uint bits)
__device__ __forceinline__ void stage_walk_params(const rt::TraceParams& P, uint32_t tid) {
    if (tid < 3u) {
        const uint32_t stride = tid == 0u ? 1u : tid == 1u ? P.grid.n[0] : P.grid.n[0] * P.grid.n[1];
        s_walk_axis[tid] = make_float4(P.grid.cs[tid], P.grid.gmin[tid], __uint_as_float(stride),
                                       __uint_as_float(P.grid.n[tid]));
        s_walk_entry[tid] = make_float4(P.grid.lo_m[tid], P.grid.hi_m[tid], P.grid.inv_cs[tid],
                                        __uint_as_float(P.grid.n[tid] - 1u));
    }
    if (tid == 3u) s_walk_slack = make_float2(P.cull_near_abs, P.cull_abs);
}

// The camera-batch kernel's camera-origin terms (rt_trace_batch.h stage_camera_terms, its only
// writer; read by setup_ray<.., CAMERA> and grid_walk<.., CAMERA>): every camera ray of a pinhole_lf
// launch starts at cam.lf, so what a segment's setup computes from the origin alone is the same for
// every generation batch of the frame.
//   [0..3] {oc.x, oc.y, oc.z, c} of the first four big spheres: oc = lf - centre, c = |oc|^2 - r^2
//   [4..6] per axis the grid's entry box from lf: (lo_m - lf, hi_m - lf, inv_cs, n - 1 as uint bits)
// The rest of its 1 KB is spare (rt_internal.h kBatchCamTabBytes).
__shared__ float4 s_cam_tab[rt::kBatchCamTabBytes / 16u];

// One DDA step of the grid walks: the axis whose boundary comes first (x before y before z on
// ties; tm = the smallest boundary t). Only the stepped coordinate can leave the grid (false:
// the ray left). The new boundary's t is recomputed from the cell coordinate, never accumulated.
__device__ __forceinline__ bool dda_step(float tm, float& tx, float& ty, float& tz, int& cx, int& cy, int& cz,
                                         int sx, int sy, int sz, uint32_t& cell, V3 o, V3 inv) {
    const bool mx = tx == tm, my = !mx && ty == tm, mz = !mx && !my;
    const float4 ax = s_walk_axis[mx ? 0 : my ? 1 : 2];
    const int s = mx ? sx : my ? sy : sz;
    const int c = (mx ? cx : my ? cy : cz) + s;
    if (uint32_t(c) >= __float_as_uint(ax.w)) return false;
    cx = mx ? c : cx;
    cy = my ? c : cy;
    cz = mz ? c : cz;
    cell = s > 0 ? cell + __float_as_uint(ax.z) : cell - __float_as_uint(ax.z);
    const float ok = mx ? o.x : my ? o.y : o.z, ik = mx ? inv.x : my ? inv.y : inv.z;
    const float tnew = (__builtin_fmaf(float(c + (s > 0 ? 1 : 0)), ax.x, ax.y) - ok) * ik;
    tx = mx ? tnew : tx;
    ty = my ? tnew : ty;
    tz = mz ? tnew : tz;
    return true;
}

// dda_step for a grid one cell thick in y (every ray is in cell row 0): the same cells in the same
// order. With one y cell a y step always leaves the grid, so the walk ends where dda_step would
// return false; only x and z step (x before z on ties, as there).
__device__ __forceinline__ bool dda_step_xz(float tm, float& tx, float ty, float& tz, int& cx, int& cz, int sx,
                                            int sz, uint32_t& cell, V3 o, V3 inv) {
    const bool mx = tx == tm;
    if (!mx && ty == tm) return false;
    const float4 ax = s_walk_axis[mx ? 0 : 2];
    const int s = mx ? sx : sz;
    const int c = (mx ? cx : cz) + s;
    if (uint32_t(c) >= __float_as_uint(ax.w)) return false;
    cx = mx ? c : cx;
    cz = mx ? cz : c;
    cell = s > 0 ? cell + __float_as_uint(ax.z) : cell - __float_as_uint(ax.z);
    const float ok = mx ? o.x : o.z, ik = mx ? inv.x : inv.z;
    const float tnew = (__builtin_fmaf(float(c + (s > 0 ? 1 : 0)), ax.x, ax.y) - ok) * ik;
    tx = mx ? tnew : tx;
    tz = mx ? tz : tnew;
    return true;
}

// Cull limit of a closest-so-far t: best + cull_abs + cull_rel best, with
// the smaller absolute slack of grid walks for t <= cull_near_t (rt_api.cpp; -1 elsewhere).
__device__ __forceinline__ float cull_limit(const rt::TraceParams& P, float t) {
    const float* slack = reinterpret_cast<const float*>(&s_walk_slack);
    const float abs_slack = slack[t <= P.cull_near_t ? 0 : 1];
    return fminf(__builtin_fmaf(t, P.cull_rel, t + abs_slack), 10000.0f);
}

// Four spheres at once (a leaf, or a batch of big spheres): the discriminants of all four are
// computed branch-free, then each lane loops over only ITS candidates (D >= 0). Inside the loop
// sits the expensive exact part (correctly rounded sqrt); t2 is computed only when t1 < tmin. The
// AABB gate is not tested here: only the segment's winner is gated, once (winner_gated).
// Candidates are accepted by (t, lowest index), so the visit order of leaves does not matter: the
// result is the brute-force closest hit. The loop reloads a candidate's record
// (rec_of, from LDS or L2) and recomputes its b and D (the same operations, so the same bits)
// instead of keeping four records and eight partial results live across it: this loop is where
// the trace kernels' register pressure peaks, and 24 fewer live VGPRs there let them run at 6
// waves per SIMD without spilling (1080p / 1000 spp: 164.7 -> 155.9 ms).
template <typename RecOf, typename IdOf>
__device__ __forceinline__ void test4(const float4 s0, const float4 s1, const float4 s2, const float4 s3,
                                      RecOf rec_of, IdOf id_of, V3 o, V3 d, V3 inv, float a, float ia,
                                      float& best, uint32_t& bi, float& limit, const rt::TraceParams& P) {
    const float4 sv[4] = {s0, s1, s2, s3};
    uint32_t cand = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float rr = sv[k].w * sv[k].w;
        const float ocx = o.x - sv[k].x, ocy = o.y - sv[k].y, ocz = o.z - sv[k].z;
        const float b = __builtin_fmaf(ocz, d.z, __builtin_fmaf(ocy, d.y, ocx * d.x));
        const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
        cand |= (__builtin_fmaf(b, b, -(a * c)) >= 0.0f && !behind(b, c) ? 1u : 0u) << k;
    }
    while (cand) {
        UTIL(2, true);
        const uint32_t k = __builtin_ctz(cand);
        cand &= cand - 1u;
        const float4 sp = rec_of(k);
        const float rr = sp.w * sp.w;
        const float ocx = o.x - sp.x, ocy = o.y - sp.y, ocz = o.z - sp.z;
        const float b = __builtin_fmaf(ocz, d.z, __builtin_fmaf(ocy, d.y, ocx * d.x));
        const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
        const float D = __builtin_fmaf(b, b, -(a * c));
        const float sq = sqrt_cr(D);
        float t = (-b - sq) * ia;
        if (!(t >= T_MIN)) t = (-b + sq) * ia;     // report t1 if t1 >= tmin, else t2
        if (t >= T_MIN && t <= best) {
            const uint32_t id = id_of(k);
            if (t < best || id < bi) {   // AABB gate deferred to the segment's winner (winner_gated)
                best = t;
                bi = id;
                limit = cull_limit(P, t);
            }
        }
    }
}

// One sphere (a grid cell's reference {cx, cy, cz, r^2}): test4's arithmetic for a single record,
// with r*r precomputed by the grid build (the same binary32 product). IdAt yields the sphere id
// when a candidate needs it (an LDS read, or a value loaded with the record from L2); ID_READY:
// the id is already in a register, so the two acceptance tests fold into one branch.
template <bool ID_READY = false, typename IdAt>
__device__ __forceinline__ void test1(const float4 sp, IdAt id_at, V3 o, V3 d, V3 inv,
                                      float a, float ia, float& best, uint32_t& bi, float& limit,
                                      const rt::TraceParams& P) {
    const float rr = sp.w;
    const float ocx = o.x - sp.x, ocy = o.y - sp.y, ocz = o.z - sp.z;
    const float b = __builtin_fmaf(ocz, d.z, __builtin_fmaf(ocy, d.y, ocx * d.x));
    const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
    const float D = __builtin_fmaf(b, b, -(a * c));
    if (D >= 0.0f && !behind(b, c)) {
        UTIL(2, true);
        const float sq = sqrt_cr(D);
        float t = (-b - sq) * ia;
        if (!(t >= T_MIN)) t = (-b + sq) * ia;     // report t1 if t1 >= tmin, else t2
#ifdef RT_UTIL
        {   // grid walks: what the candidate tails find (12 beyond the closest so far, 13 the current
            // winner again from a later cell, 14 both roots below tmin, 15 passes no lane needed)
            const uint32_t idd = id_at();
            UTIL(12, t > best);
            UTIL(13, t == best && idd == bi);
            UTIL(14, !(t >= T_MIN));
            if (!__ballot((t >= T_MIN) & ((t < best) | ((t == best) & (idd < bi))))) UTIL(15, true);
        }
#endif
        if (ID_READY) {
            const uint32_t id = id_at();
            if ((t >= T_MIN) & (t <= best) & ((t < best) | (id < bi))) {   // one predicate, one branch
                best = t;
                bi = id;
                limit = cull_limit(P, t);
            }
        } else if (t >= T_MIN && t <= best) {
            const uint32_t id = id_at();
            if (t < best || id < bi) {   // AABB gate deferred to the segment's winner (winner_gated)
                best = t;
                bi = id;
                limit = cull_limit(P, t);
            }
        }
    }
}

// Brute force: every lane tests every sphere. The sphere index is wave-uniform, so the geometry
// comes through the scalar cache: 8 spheres (128 B) per iteration as two s_load_dwordx16 issued
// before any of the 8 tests, feeding the VALU as SGPR operands (13 VALU per sphere, no VGPR
// loads, no LDS). The host pads geom to a multiple of 8 with spheres that can never report.
template <bool GATE>
__device__ __forceinline__ void closest_brute(const rt::TraceParams& P, V3 o, V3 d, V3 inv, float a,
                                              float ia, float& best, uint32_t& bi) {
    // Constant address space: wave-uniform loads through it are emitted as s_load (the 32
    // floats of one batch merge into two s_load_dwordx16).
    typedef const __attribute__((address_space(4))) float* ConstF;
    const ConstF g = (ConstF)(P.geom);
    const uint32_t nb = (P.n_spheres + 7u) >> 3;
    for (uint32_t ib = 0; ib < nb; ++ib) {
        float b[32];
#pragma unroll
        for (uint32_t k = 0; k < 32; ++k) b[k] = g[ib * 32u + k];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            test_sphere<GATE>(b[4 * k], b[4 * k + 1], b[4 * k + 2], b[4 * k + 3], P.radius, o, d, inv, a, ia,
                        ib * 8u + k, best, bi);
    }
}

// A segment's ray and its closest hit so far: the state every walk form carries.
struct Ray {
    V3 o, d, inv;          // origin, direction, 1/d (the AABB gate's own reciprocals)
    float a, ia;           // dot(d, d) and its reciprocal
    float limit;           // node cull limit: min(best + cull_abs + cull_rel * best, tmax)
    float best;
    uint32_t bi;           // closest so far
    bool walk;             // the segment has a tree to walk
};

}  // namespace
