// rt_trace_grid_coop.h — the wave-cooperative grid walk (LAYOUT_GRID_COOP; device
// only): the wave scans, grid_walk_coop and its LDS arrays. The quadratic is
// shaders/shader.rint:44-60 as rt_trace_prims.h restates it; the regrouping has no reference
// counterpart.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"
#include "rt_trace_grid.h"
#include "rt_trace_prims.h"

using namespace rtd;

namespace {

// ---- wave-cooperative grid walk (LAYOUT_GRID_COOP) ---------------------------
// Wave64 inclusive scans through DPP: row_shr 1/2/4/8 inside each 16-lane row (zero fill), then
// row_bcast:15 (lane 15 of rows 0 / 2 into rows 1 / 3) and row_bcast:31 (lane 31 into rows 2, 3).
// Every lane of the wave must be active (exec full): DPP reads disabled lanes as the fill value.
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xf, 0xf, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xf, 0xf, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xf, 0xf, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xf, 0xf, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xa, 0xf, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xc, 0xf, false));
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xf, 0xf, false)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xf, 0xf, false)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xf, 0xf, false)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xf, 0xf, false)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xa, 0xf, false)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xc, 0xf, false)));
    return v;
}

// Per wave (64 slots of its block's arrays): the rays of the segment (o, a | d, 1/a), the closest
// hit so far as a (t bits, sphere id) key, and the slot markers of one pass.
__shared__ float4 s_coop_ray[2 * RT_TRACE_BLOCK];
__shared__ unsigned long long s_coop_key[RT_TRACE_BLOCK];
__shared__ uint32_t s_coop_mark[RT_TRACE_BLOCK];
static_assert(sizeof(s_coop_ray) + sizeof(s_coop_key) + sizeof(s_coop_mark) == rt::kCoopLdsBytes, "rt_internal.h");

// The grid walk of grid_walk with the reference tests of a wave's rays spread over all 64 lanes.
// Rounds: every walking lane takes its current cell's n references; an exclusive scan of n gives
// each ray its run [start, start + n) of the round's `total` (ray, reference) pairs, which the
// wave tests in ceil(total / 64) passes with every lane busy instead of max-over-lanes passes at
// one reference per lane. A pass finds each slot's ray by a max-scan of the runs' start markers;
// a candidate lowers its ray's key by an LDS 64-bit atomic minimum. t >= tmin > 0, so the float
// bits order like the values and the u64 minimum of (t bits << 32 | id) is exactly the walks'
// (t, lowest id) rule: the order of tests cannot change the result. After the passes each ray
// reads its key, updates its cull limit and takes its DDA step, as grid_walk does after a cell:
// the cells visited, the references tested and the closest hit are grid_walk's. Called with every
// lane of the wave (tracing or not), never inside divergent control flow.
template <bool COUNT>
__device__ __forceinline__ void grid_walk_coop(const rt::TraceParams& P, const uint32_t* __restrict__ cstart,
                                               const float4* __restrict__ rec, const uint32_t* __restrict__ ids,
                                               Ray& r, bool tracing, uint32_t& n_cell, uint32_t& n_sph) {
    const rt::GridInfo& G = P.grid;
    const uint32_t lane = lane_id();
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    float4* const rayA = s_coop_ray + wave0;
    float4* const rayB = s_coop_ray + RT_TRACE_BLOCK + wave0;
    unsigned long long* const key = s_coop_key + wave0;
    uint32_t* const mark = s_coop_mark + wave0;
    bool walking = tracing && r.walk;
    int cx = 0, cy = 0, cz = 0, sx = 0, sy = 0, sz = 0;
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;
    uint32_t cell = 0;
    if (walking) {   // entry cell and DDA state: grid_walk's arithmetic
        const float x0 = (G.lo_m[0] - r.o.x) * r.inv.x, x1 = (G.hi_m[0] - r.o.x) * r.inv.x;
        const float y0 = (G.lo_m[1] - r.o.y) * r.inv.y, y1 = (G.hi_m[1] - r.o.y) * r.inv.y;
        const float z0 = (G.lo_m[2] - r.o.z) * r.inv.z, z1 = (G.hi_m[2] - r.o.z) * r.inv.z;
        const float tn = fmaxf(fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1)), T_MIN);
        const float tf = fminf(fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)), r.limit);
        walking = tn <= tf;
        if (walking) {
            auto cell_of = [&](float p, int k) {
                const int c = int(floorf((p - G.gmin[k]) * G.inv_cs[k]));
                return min(max(c, 0), int(G.n[k]) - 1);
            };
            cx = cell_of(__builtin_fmaf(tn, r.d.x, r.o.x), 0);
            cy = cell_of(__builtin_fmaf(tn, r.d.y, r.o.y), 1);
            cz = cell_of(__builtin_fmaf(tn, r.d.z, r.o.z), 2);
            sx = r.d.x > 0.0f ? 1 : (r.d.x < 0.0f ? -1 : 0);
            sy = r.d.y > 0.0f ? 1 : (r.d.y < 0.0f ? -1 : 0);
            sz = r.d.z > 0.0f ? 1 : (r.d.z < 0.0f ? -1 : 0);
            auto bound_t = [&](int c, int s, int k, float o, float inv) {
                const float plane = __builtin_fmaf(float(c + (s > 0 ? 1 : 0)), G.cs[k], G.gmin[k]);
                return s == 0 ? __builtin_inff() : (plane - o) * inv;
            };
            tx = bound_t(cx, sx, 0, r.o.x, r.inv.x);
            ty = bound_t(cy, sy, 1, r.o.y, r.inv.y);
            tz = bound_t(cz, sz, 2, r.o.z, r.inv.z);
            cell = (uint32_t(cz) * G.n[1] + uint32_t(cy)) * G.n[0] + uint32_t(cx);
            rayA[lane] = make_float4(r.o.x, r.o.y, r.o.z, r.a);
            rayB[lane] = make_float4(r.d.x, r.d.y, r.d.z, r.ia);
            key[lane] = (static_cast<unsigned long long>(__float_as_uint(r.best)) << 32) | r.bi;
        }
    }
    while (__ballot(walking)) {
        uint32_t b = 0u, n = 0u;
        if (walking) {
            b = cstart[cell];
            n = cstart[cell + 1] - b;
            if (COUNT) { n_cell++; n_sph += n; }
        }
        const uint32_t incl = wave_scan_add(n);
        const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
        const uint32_t start = incl - n;
        const uint32_t off = b - start;   // reference of slot s of this ray: s + off
        uint32_t carry = 0u;              // marker (owner + 1) of the last slot of the previous pass
        for (uint32_t base = 0; base < total; base += 64u) {
            mark[lane] = 0u;
            lane_order();
            if (n != 0u && start - base < 64u) mark[start - base] = lane + 1u;
            lane_order();
            const uint32_t m = max(wave_scan_max(mark[lane]), carry);
            carry = __builtin_amdgcn_readlane(m, 63);
            const uint32_t L = (m - 1u) & 63u;   // the slot's ray
            const uint32_t offL = __shfl(off, int(L));
            const uint32_t s = base + lane;
            UTIL(1, s < total);
            if (s < total) {
                const uint32_t j = s + offL;
                const float4 A = rayA[L], B = rayB[L], sp = rec[j];
                const float rr = sp.w;   // grid record: r^2
                const float ocx = A.x - sp.x, ocy = A.y - sp.y, ocz = A.z - sp.z;
                const float bb = __builtin_fmaf(ocz, B.z, __builtin_fmaf(ocy, B.y, ocx * B.x));
                const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - rr;
                const float D = __builtin_fmaf(bb, bb, -(A.w * c));
                if (D >= 0.0f && !behind(bb, c)) {
                    UTIL(2, true);
                    const float sq = sqrt_cr(D);
                    float t = (-bb - sq) * B.w;
                    if (!(t >= T_MIN)) t = (-bb + sq) * B.w;   // report t1 if t1 >= tmin, else t2
                    if (t >= T_MIN) {
                        const unsigned long long k = (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | ids[j];
                        __hip_atomic_fetch_min(&key[L], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    }
                }
            }
            lane_order();
        }
        if (walking) {
            const unsigned long long k = key[lane];
            r.best = __uint_as_float(uint32_t(k >> 32));
            r.bi = uint32_t(k);
            r.limit = cull_limit(P, r.best);
            UTIL(0, true);
            // DDA step (grid_walk): the axis whose boundary comes first, x before y before z on ties
            const float tm = fminf(fminf(tx, ty), tz);
            if (!(tm <= r.limit)) {
                walking = false;   // the next cell starts beyond every closer candidate
            } else {
                walking = dda_step(tm, tx, ty, tz, cx, cy, cz, sx, sy, sz, cell, r.o, r.inv);
            }
        }
    }
}

}  // namespace
