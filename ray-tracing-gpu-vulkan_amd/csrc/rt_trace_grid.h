// rt_trace_grid.h — the uniform-grid walk, one ray per lane (device only): grid_walk for the grid in
// LDS or in L2, in its general and its one-layer form, and lane_order. Stands in for the driver
// traversal of the reference's acceleration structure (src/vulkan.h:395-554), as rt_grid.h says;
// the reference tests are rt_trace_prims.h's (shaders/shader.rint:44-60).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"
#include "rt_trace_prims.h"

using namespace rtd;

namespace {

// Uniform-grid walk (ACCEL_GRID, rt_grid.h): a 3D DDA from the ray's entry into the grid box
// (widened by the registration margin, over [tmin, limit], in the AABB gate's arithmetic) through
// the cells in order of t, testing each cell's references, until the next cell starts beyond the
// cull limit or the ray leaves the grid. Every cell boundary's t is computed afresh from the cell
// coordinate (no accumulated rounding), so the cells visited cover the ray up to rounding distance
// of the boundaries, which the margin covers. Ties step one axis at a time (an
// extra cell, never a skipped one).
// CAMERA (the camera-batch kernel's generation batches): every ray starts at cam.lf, so the entry
// box comes as (lo_m - lf, hi_m - lf) from s_cam_tab, the six subtractions done once per block by
// the same binary32 operation. A lane whose origin is NaN (lens sample (0, 0)) needs no special
// case: its d and so its inv are NaN, the six products are NaN with either operand, and tn, tf come
// out as T_MIN and r.limit as they do from (lo - NaN) * NaN (fmaxf / fminf drop a NaN operand,
// whatever its payload). Everything past the entry test reads r.o itself.
template <bool COUNT, bool PAIRS, bool FLAT = false, bool CAMERA = false>
__device__ __forceinline__ void grid_walk(const rt::TraceParams& P, const uint32_t* __restrict__ cstart,
                                          const float4* __restrict__ rec, const uint32_t* __restrict__ ids,
                                          Ray& r, uint32_t& n_cell, uint32_t& n_sph, uint32_t& n_empty) {
    // grid parameters from the block's LDS tables (stage_walk_params), not from the kernel arguments
    const float4 ex = CAMERA ? s_cam_tab[4] : s_walk_entry[0], ey = CAMERA ? s_cam_tab[5] : s_walk_entry[1],
                 ez = CAMERA ? s_cam_tab[6] : s_walk_entry[2];
    const float4 axx = s_walk_axis[0], axy = s_walk_axis[1], axz = s_walk_axis[2];
    const float lo0 = ex.x, lo1 = ey.x, lo2 = ez.x, hi0 = ex.y, hi1 = ey.y, hi2 = ez.y;
    const float ics[3] = {ex.z, ey.z, ez.z}, gmn[3] = {axx.y, axy.y, axz.y}, csz[3] = {axx.x, axy.x, axz.x};
    const int nm1[3] = {int(__float_as_uint(ex.w)), int(__float_as_uint(ey.w)), int(__float_as_uint(ez.w))};
    const uint32_t n0 = __float_as_uint(axx.w), n1 = __float_as_uint(axy.w);
    const float x0 = (CAMERA ? lo0 : lo0 - r.o.x) * r.inv.x, x1 = (CAMERA ? hi0 : hi0 - r.o.x) * r.inv.x;
    const float y0 = (CAMERA ? lo1 : lo1 - r.o.y) * r.inv.y, y1 = (CAMERA ? hi1 : hi1 - r.o.y) * r.inv.y;
    const float z0 = (CAMERA ? lo2 : lo2 - r.o.z) * r.inv.z, z1 = (CAMERA ? hi2 : hi2 - r.o.z) * r.inv.z;
    const float tn = fmaxf(fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1)), T_MIN);
    const float tf = fminf(fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)), r.limit);
    if (!(tn <= tf)) return;
    // entry cell (clamped: a point rounded just outside belongs to the border cell)
    auto cell_of = [&](float p, int k) {
        const int c = int(floorf((p - gmn[k]) * ics[k]));
        return min(max(c, 0), nm1[k]);
    };
    int cx = cell_of(__builtin_fmaf(tn, r.d.x, r.o.x), 0);
    int cy = FLAT ? 0 : cell_of(__builtin_fmaf(tn, r.d.y, r.o.y), 1);
    int cz = cell_of(__builtin_fmaf(tn, r.d.z, r.o.z), 2);
    const int sx = r.d.x > 0.0f ? 1 : (r.d.x < 0.0f ? -1 : 0);
    const int sy = r.d.y > 0.0f ? 1 : (r.d.y < 0.0f ? -1 : 0);
    const int sz = r.d.z > 0.0f ? 1 : (r.d.z < 0.0f ? -1 : 0);
    // t of the boundary ahead on each axis (+inf on an axis the ray does not move along)
    auto bound_t = [&](int c, int s, int k, float o, float inv) {
        const float plane = __builtin_fmaf(float(c + (s > 0 ? 1 : 0)), csz[k], gmn[k]);
        return s == 0 ? __builtin_inff() : (plane - o) * inv;
    };
    float tx = bound_t(cx, sx, 0, r.o.x, r.inv.x);
    float ty = bound_t(cy, sy, 1, r.o.y, r.inv.y);
    float tz = bound_t(cz, sz, 2, r.o.z, r.inv.z);
    // linear cell index (a step adds the stepped axis's stride, dda_step)
    uint32_t cell = FLAT ? uint32_t(cz) * n0 + uint32_t(cx) : (uint32_t(cz) * n1 + uint32_t(cy)) * n0 + uint32_t(cx);
    // One-layer grid walked from L2 (config 5): the DDA steps before the cell's references are
    // tested (the step does not depend on them; the cull test still uses this cell's exit t and the
    // limit they leave), so the next cell's two offsets are requested before this cell's records
    // and arrive while they are tested: one dependent L2 round trip per cell instead of two, the
    // same cells and references in the same order. Config 5 -0.3 % (1 000 spp) / -0.9 % (100 spp),
    // no new spills.
    if constexpr (FLAT && PAIRS) {
        uint32_t b = cstart[cell], e = cstart[cell + 1];
        for (;;) {
            const float tm = fminf(fminf(tx, ty), tz);
            uint32_t ncell = cell;   // unchanged when the step leaves the grid: a valid address
            const bool more = dda_step_xz(tm, tx, ty, tz, cx, cz, sx, sz, ncell, r.o, r.inv);
            const uint32_t nb = cstart[ncell], ne = cstart[ncell + 1];
            if (COUNT) {
                n_cell++;
                n_empty += b == e ? 1u : 0u;
            }
            uint32_t j = b;
            for (; j + 1 < e; j += 2) {
                UTIL(1, true);
                const float4 s0 = rec[j], s1 = rec[j + 1];
                const uint32_t i0 = ids[j], i1 = ids[j + 1];
                test1<true>(s0, [&] { return i0; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
                test1<true>(s1, [&] { return i1; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
                if (COUNT) n_sph += 2;
            }
            if (j < e) {
                UTIL(1, true);
                const float4 s0 = rec[j];
                const uint32_t i0 = ids[j];
                test1<true>(s0, [&] { return i0; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
                if (COUNT) n_sph++;
            }
            UTIL(0, true);
            if (!(tm <= r.limit) || !more) break;
            b = nb;
            e = ne;
            cell = ncell;
        }
        return;
    }
    for (;;) {
        // the cell's reference run [b, e): from L2 through one address, so both offsets come in one
        // 8-byte load (config 5 -1.0 %); the LDS pair is one ds_read2 either way
        const uint32_t* cp = cstart + cell;
        const uint32_t b = PAIRS ? cp[0] : cstart[cell], e = PAIRS ? cp[1] : cstart[cell + 1];
        if (COUNT) {
            n_cell++;
            n_empty += b == e ? 1u : 0u;
        }
        uint32_t j = b;
        if (PAIRS) {   // references from L2: two at a time (two record loads in flight; config 5 -3.5 %)
          // the ids are loaded with the records (one L2 round trip instead of a second, dependent
          // one for every candidate that passes the t test)
          for (; j + 1 < e; j += 2) {
            UTIL(1, true);
            const float4 s0 = rec[j], s1 = rec[j + 1];
            const uint32_t i0 = ids[j], i1 = ids[j + 1];
            test1<true>(s0, [&] { return i0; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
            test1<true>(s1, [&] { return i1; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
            if (COUNT) n_sph += 2;
          }
          if (j < e) {
            UTIL(1, true);
            const float4 s0 = rec[j];
            const uint32_t i0 = ids[j];
            test1<true>(s0, [&] { return i0; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
            if (COUNT) n_sph++;
            ++j;
          }
        }
        if (!PAIRS && j < e) {   // LDS: two records in flight, no register copies (unrolled by two)
            float4 A = rec[j], B;
            for (;;) {
                UTIL(1, true);
                B = rec[j + 1];   // one past the run: the next cell's record or the id array (LDS)
                test1(A, [&] { return ids[j]; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
                if (COUNT) n_sph++;
                if (++j >= e) break;
                UTIL(1, true);
                A = rec[j + 1];
                test1(B, [&] { return ids[j]; }, r.o, r.d, r.inv, r.a, r.ia, r.best, r.bi, r.limit, P);
                if (COUNT) n_sph++;
                if (++j >= e) break;
            }
        }
        UTIL(0, true);
        const float tm = fminf(fminf(tx, ty), tz);
        if (!(tm <= r.limit)) break;   // the next cell starts beyond every closer candidate
        if (FLAT) {
            if (!dda_step_xz(tm, tx, ty, tz, cx, cz, sx, sz, cell, r.o, r.inv)) break;
        } else if (!dda_step(tm, tx, ty, tz, cx, cy, cz, sx, sy, sz, cell, r.o, r.inv)) {
            break;
        }
    }
}

// Compiler-only ordering of LDS accesses made by different lanes of one wave: the LDS executes a
// wave's instructions in issue order, so no wait or barrier is needed, only no reordering.
__device__ __forceinline__ void lane_order() { asm volatile("" ::: "memory"); }

}  // namespace
