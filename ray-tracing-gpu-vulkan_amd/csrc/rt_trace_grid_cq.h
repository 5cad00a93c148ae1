// rt_trace_grid_cq.h — the grid walk with a wave-wide candidate queue (LAYOUT_GRID_CQ, DESIGN.md
// §4.9; device only): grid_walk_cq and its LDS arrays. The quadratic is shaders/shader.rint:44-60
// as rt_trace_prims.h restates it; the queue has no reference counterpart.
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

// ---- wave-wide candidate queue (LAYOUT_GRID_CQ) --------------------------------
// The LDS grid walk with the candidate tails (sqrt, roots, acceptance) taken out of the divergent
// reference loop: a reference whose discriminant passes is pushed as (lane, reference) into a
// per-wave LDS queue (ballot ranks), and at the end of each cell the wave's walking lanes resolve
// the queue together, every lane taking entries, before any of them takes its DDA step. An entry's
// ray comes from its owner lane by ds_bpermute (every owner is active at the flush: it pushed in
// this cell), its candidate lowers the owner's (t bits, id) key by an LDS 64-bit atomic minimum
// (t >= tmin > 0: the u64 minimum is the walks' (t, lowest id) rule). Per-lane queue overflow
// (more than kCqCap entries in one cell) falls back to the lane's own tail. The cells visited, the
// references tested and the closest hit are grid_walk's: bit-exact.
constexpr uint32_t kCqCap = 128;   // queue entries per wave
__shared__ uint32_t s_cq_q[kCqCap * (RT_TRACE_BLOCK / 64)];
__shared__ unsigned long long s_cq_key[RT_TRACE_BLOCK];
__shared__ uint32_t s_cq_n[RT_TRACE_BLOCK / 64];
static_assert(sizeof(s_cq_q) + sizeof(s_cq_key) + sizeof(s_cq_n) == rt::kCqLdsBytes, "rt_internal.h");

template <bool COUNT>
__device__ __forceinline__ void grid_walk_cq(const rt::TraceParams& P, const uint32_t* __restrict__ cstart,
                                             const float4* __restrict__ rec, const uint32_t* __restrict__ ids,
                                             Ray& r, uint32_t& n_cell, uint32_t& n_sph, uint32_t& n_empty) {
    const rt::GridInfo& G = P.grid;
    const float x0 = (G.lo_m[0] - r.o.x) * r.inv.x, x1 = (G.hi_m[0] - r.o.x) * r.inv.x;
    const float y0 = (G.lo_m[1] - r.o.y) * r.inv.y, y1 = (G.hi_m[1] - r.o.y) * r.inv.y;
    const float z0 = (G.lo_m[2] - r.o.z) * r.inv.z, z1 = (G.hi_m[2] - r.o.z) * r.inv.z;
    const float tn = fmaxf(fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1)), T_MIN);
    const float tf = fminf(fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)), r.limit);
    if (!(tn <= tf)) return;
    auto cell_of = [&](float p, int k) {
        const int c = int(floorf((p - G.gmin[k]) * G.inv_cs[k]));
        return min(max(c, 0), int(G.n[k]) - 1);
    };
    int cx = cell_of(__builtin_fmaf(tn, r.d.x, r.o.x), 0);
    int cy = cell_of(__builtin_fmaf(tn, r.d.y, r.o.y), 1);
    int cz = cell_of(__builtin_fmaf(tn, r.d.z, r.o.z), 2);
    const int sx = r.d.x > 0.0f ? 1 : (r.d.x < 0.0f ? -1 : 0);
    const int sy = r.d.y > 0.0f ? 1 : (r.d.y < 0.0f ? -1 : 0);
    const int sz = r.d.z > 0.0f ? 1 : (r.d.z < 0.0f ? -1 : 0);
    auto bound_t = [&](int c, int s, int k, float o, float inv) {
        const float plane = __builtin_fmaf(float(c + (s > 0 ? 1 : 0)), G.cs[k], G.gmin[k]);
        return s == 0 ? __builtin_inff() : (plane - o) * inv;
    };
    float tx = bound_t(cx, sx, 0, r.o.x, r.inv.x);
    float ty = bound_t(cy, sy, 1, r.o.y, r.inv.y);
    float tz = bound_t(cz, sz, 2, r.o.z, r.inv.z);
    uint32_t cell = (uint32_t(cz) * G.n[1] + uint32_t(cy)) * G.n[0] + uint32_t(cx);
    const uint32_t lane = lane_id();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* const q = s_cq_q + wave * kCqCap;
    unsigned long long* const key = s_cq_key + wave * 64u;
    for (;;) {
        const uint32_t b = cstart[cell], e = cstart[cell + 1];
        if (COUNT) {
            n_cell++;
            n_empty += b == e ? 1u : 0u;
        }
        s_cq_n[wave] = 0u;   // every active lane writes the same value
        lane_order();
        uint32_t qn = 0u;   // equal on every lane still in the reference loop (they ran the same pushes)
        for (uint32_t j = b; j < e; ++j) {
            UTIL(1, true);
            const float4 sp = rec[j];
            const float ocx = r.o.x - sp.x, ocy = r.o.y - sp.y, ocz = r.o.z - sp.z;
            const float bb = __builtin_fmaf(ocz, r.d.z, __builtin_fmaf(ocy, r.d.y, ocx * r.d.x));
            const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - sp.w;
            const float D = __builtin_fmaf(bb, bb, -(r.a * c));
            if (COUNT) n_sph++;
            const bool cand = D >= 0.0f && !behind(bb, c);
            const unsigned long long m = __ballot(cand);
            if (m) {   // wave-uniform
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                const uint32_t slot = qn + rank;
                qn = min(qn + uint32_t(__popcll(m)), kCqCap);
                if (cand) {
                    if (rank == 0u) s_cq_n[wave] = qn;
                    if (slot < kCqCap) {
                        q[slot] = lane | (j << 6);
                    } else {   // the queue is full: this lane's own tail (rare)
                        UTIL(2, true);
                        const float sq = sqrt_cr(D);
                        float t = (-bb - sq) * r.ia;
                        if (!(t >= T_MIN)) t = (-bb + sq) * r.ia;
                        const uint32_t id = ids[j];
                        if ((t >= T_MIN) & (t <= r.best) & ((t < r.best) | (id < r.bi))) {
                            r.best = t;
                            r.bi = id;
                        }
                    }
                }
            }
        }
        lane_order();
        const uint32_t qtot = __builtin_amdgcn_readfirstlane(s_cq_n[wave]);
        if (qtot) {   // resolve the cell's candidates with every walking lane
            key[lane] = (static_cast<unsigned long long>(__float_as_uint(r.best)) << 32) | r.bi;
            lane_order();
            const unsigned long long act = __ballot(true);
            const uint32_t rk = __builtin_amdgcn_mbcnt_hi(uint32_t(act >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(act), 0u));
            const uint32_t nact = __popcll(act);
            for (uint32_t base = 0; base < qtot; base += nact) {   // wave-uniform trip count
                const uint32_t k = base + rk;
                const bool valid = k < qtot;
                const uint32_t ent = q[valid ? k : 0u];
                const int L = int(ent & 63u);
                const uint32_t jj = ent >> 6;
                const V3 o = v3(__shfl(r.o.x, L), __shfl(r.o.y, L), __shfl(r.o.z, L));
                const V3 d = v3(__shfl(r.d.x, L), __shfl(r.d.y, L), __shfl(r.d.z, L));
                const float a = __shfl(r.a, L), ia = __shfl(r.ia, L);
                UTIL(2, valid);
                const float4 sp = rec[jj];
                const uint32_t id = ids[jj];
                const float ocx = o.x - sp.x, ocy = o.y - sp.y, ocz = o.z - sp.z;
                const float bb = __builtin_fmaf(ocz, d.z, __builtin_fmaf(ocy, d.y, ocx * d.x));
                const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, ocx * ocx)) - sp.w;
                const float D = __builtin_fmaf(bb, bb, -(a * c));   // the push's D: >= 0
                const float sq = sqrt_cr(D);
                float t = (-bb - sq) * ia;
                if (!(t >= T_MIN)) t = (-bb + sq) * ia;   // report t1 if t1 >= tmin, else t2
                if (valid && t >= T_MIN)
                    __hip_atomic_fetch_min(&key[L], (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | id,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            lane_order();
            const unsigned long long kk = key[lane];
            r.best = __uint_as_float(uint32_t(kk >> 32));
            r.bi = uint32_t(kk);
        }
        r.limit = cull_limit(P, r.best);
        UTIL(0, true);
        const float tm = fminf(fminf(tx, ty), tz);
        if (!(tm <= r.limit)) break;   // the next cell starts beyond every closer candidate
        if (!dda_step(tm, tx, ty, tz, cx, cy, cz, sx, sy, sz, cell, r.o, r.inv)) break;
    }
}

}  // namespace
