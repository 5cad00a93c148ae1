// rt_trace_shade.h — the pieces of shader.rgen / rchit / rmiss shared by every kernel (device only):
//   shaders/shader.rgen:56-58, 107-115   the camera ray of a sample (camera_ray, start_sample)
//   shaders/shader.rgen:77-88, 59-60     the bounce loop's step and the sample's sum (shade_rec,
//                                        sample_end)
//   shaders/shader.rchit:38-133          normal, texture, diffuse / metal / dielectric scatter
//   shaders/shader.rmiss:13-18           constant sky
// with the hit sphere's records (HitRec) from the scene's arrays or the static LDS table (s_rec).
// Stands without the walks: the scatter probe (rt_debug_kernels.hip) includes it alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_trace_diag.h"
#include "rt_trace_units.h"

using namespace rtd;

namespace {

struct Camera { V3 lf, hor, ver, ulc, cup, crt; };

__device__ __forceinline__ Camera load_camera(const rt::TraceParams& P) {
    return Camera{v3(P.lf[0], P.lf[1], P.lf[2]), v3(P.hor[0], P.hor[1], P.hor[2]),
                  v3(P.ver[0], P.ver[1], P.ver[2]), v3(P.ulc[0], P.ulc[1], P.ulc[2]),
                  v3(P.cup[0], P.cup[1], P.cup[2]), v3(P.crt[0], P.crt[1], P.crt[2])};
}

// shader.rgen:56-58 + 107-115: camera ray of sample ps.s of the lane's unit: origin o and the
// direction before normalisation, v = to - from (the caller normalises it).
// FAST: a launch the host proved pinhole_lf for (the one-layer L2 grid kernel, lbvh_loop SPEC).
template <int MODE, bool FAST = false>
__device__ __forceinline__ void camera_ray(const rt::TraceParams& P, const Camera& cam, Path& ps, V3& o, V3& v) {
    UTIL(7, true);
    const uint32_t lx = ps.px & 0xffffu, ly = ps.px >> 16;
    const uint32_t gx = P.off_x + lx;
    const uint32_t gy = band_row(P, ly);
    if (MODE == rt::MODE_HASH) ps.seed = sample_seed_hash(ps.pixel_seed, P.sample_base + ps.s);
    else if (P.rng_counter) ps.seed = tea(ps.pixel_seed, P.sample_base + ps.s);
    float ux = float(gx) + rnd(ps.seed);
    float uy = float(gy) + rnd(ps.seed);
    // ux / size_x, correctly rounded, as one double multiply by the host's double 1/size (3 VALU
    // instead of 11): binary32 quotients lie at least 2^-49 (relative) from a binary32 rounding
    // boundary and never on one, and the double product is within 2^-52 of the quotient, so its
    // rounding to float is the correctly rounded quotient.
    ux = float(double(ux) * P.inv_size_x);
    uy = float(double(uy) * P.inv_size_y);
    const float lxr = rnd_pm1(ps.seed);
    const float lyr = rnd_pm1(ps.seed);
    V3 from;
    if (FAST || P.pinhole_lf) {   // wave-uniform (launch parameter): the reference camera (aperture 0), every
        // component of lf nonzero, crt and cup finite: rx and ry below are +-0 (or both NaN when the
        // disk sample is (0, 0)), so lf + (rx crt + ry cup) is lf itself (or NaN), without the six
        // products and sums and the 6 SGPRs of crt / cup (config 3 -0.65 %, reference stream -1.5 %,
        // config 5 -0.75 %)
        const bool nan = lxr == 0.0f && lyr == 0.0f;
        const float q = __builtin_nanf("");
        from = nan ? v3(q, q, q) : cam.lf;
    } else {
    float rx, ry;
    if (P.half_aperture != 0.0f) {   // wave-uniform (launch parameter)
        const float l2 = __builtin_sqrtf(__builtin_fmaf(lyr, lyr, lxr * lxr));
        const float il = 1.0f / l2;
        rx = P.half_aperture * (lxr * il);
        ry = P.half_aperture * (lyr * il);
    } else {
        // Pinhole (the reference camera, aperture 0): the same values without the sqrt and the
        // divide. lxr * il has the sign of lxr (il = 1/l2 > 0), so 0 * it is a zero of sign
        // sign(aperture) ^ sign(lxr); when lxr = lyr = 0 exactly, il = inf and 0 * (0 * inf) = NaN.
        const bool nan = lxr == 0.0f && lyr == 0.0f;
        const uint32_t sa = __float_as_uint(P.half_aperture) & 0x80000000u;
        rx = nan ? __builtin_nanf("") : __uint_as_float(sa ^ (__float_as_uint(lxr) & 0x80000000u));
        ry = nan ? __builtin_nanf("") : __uint_as_float(sa ^ (__float_as_uint(lyr) & 0x80000000u));
    }
    from = add(cam.lf, add(scale(rx, cam.crt), scale(ry, cam.cup)));
    }
    const V3 to = sub(add(cam.ulc, scale(ux, cam.hor)), scale(uy, cam.ver));
    o = from;
    v = sub(to, from);
    ps.thr = v3(1.0f, 1.0f, 1.0f);
    ps.depth = 0;
}

// First camera ray of a unit just taken. Returns false when the unit has no samples (spp = 0:
// stored at once); later samples start inside shade().
template <int MODE, bool LSUM, bool FAST = false>
__device__ __forceinline__ bool start_sample(const rt::TraceParams& P, const Camera& cam, Path& ps,
                                             V3& o, V3& d) {
    if (ps.s >= ps.s_end) {
        finish_unit<MODE, LSUM>(P, ps);
        return false;
    }
    V3 v;
    if constexpr (MODE == rt::MODE_PROBE) {   // the unit's texel is a ray of the caller's batch
        const float* q = P.probe_rays + 6u * (size_t(ps.px >> 16) * P.band_w + (ps.px & 0xffffu));
        o = v3(q[0], q[1], q[2]);
        v = v3(q[3], q[4], q[5]);
        ps.depth = 0;
    } else if constexpr (MODE == rt::MODE_FEATURES) {   // sample s of the pixel is HASH's camera ray
        camera_ray<rt::MODE_HASH, FAST>(P, cam, ps, o, v);
    } else {
        camera_ray<MODE, FAST>(P, cam, ps, o, v);
    }
    d = normalize(v);
    return true;
}

// The sample's colour added to the unit's sum (shader.rgen:85-88, 59-60).
template <int MODE, bool LSUM>
__device__ __forceinline__ void sample_end(const rt::TraceParams& P, Path& ps, const V3 col) {
    ps.s++;
    if (MODE == rt::MODE_HASH) {
        ps.qx += sample_fixed(col.x);
        ps.qy += sample_fixed(col.y);
        ps.qz += sample_fixed(col.z);
        // a partial never spans a multiple of kFixedFlush samples: <= kFixedFlush * 2^24 < 2^32
        if ((ps.s & (rt::kFixedFlush - 1u)) == 0u) flush_fixed<LSUM>(P, ps);
    } else {
        ps.sx += double(col.x);
        ps.sy += double(col.y);
        ps.sz += double(col.z);
    }
}

// The hit sphere's records shade() reads: its geometry record and its two material records.
struct HitRec {
    float4 g, m0, m1;
};

__device__ __forceinline__ HitRec load_hit(const float4* __restrict__ geom4, const float4* __restrict__ mat4,
                                           uint32_t bi) {
    return HitRec{geom4[bi], mat4[2 * bi], mat4[2 * bi + 1]};
}

// The REC grid kernels' gate and shading records, {c, r} + the material record of a sphere side by
// side (48 B), in a static LDS table at a fixed address: a record's address is 48 bi with no base
// register (the dynamic table's two bases were spilled SGPRs reloaded every segment: config 3
// -0.5 %). Scenes of at most kRecStatic spheres (the host's choice of the form).
__shared__ float4 s_rec[3 * rt::kRecStatic];
__device__ __forceinline__ HitRec load_hit_rec(uint32_t bi) {
    return HitRec{s_rec[3 * bi], s_rec[3 * bi + 1], s_rec[3 * bi + 2]};
}

// shader.rchit:38-133 / shader.rmiss:13-18 + shader.rgen:77-88 for one finished trace. When the
// sample ends, its colour is added to the unit's sum and the unit's next sample starts here
// (`fresh`): the scattered and the camera direction share one normalisation, and the loop head's
// sample start runs only for units just taken. Returns true when the lane traces again (o, d hold
// the next ray), false when its unit's samples are done.
// hr: the records of sphere bi (load_hit), loaded by the caller so that they can travel with the
// winner gate's loads (lbvh_loop); unused on a miss.
// ALT (the camera-batch kernel's generation batches): *alt is set to 1 where the checker texture
// chose colour 1 (the caller clears it), so the caller knows which material record att came from.
// LEAN (the camera-batch kernel's segments only; every other caller's code is what it was): sd and p
// have no value on a miss, where nothing reads them (a miss never scatters, and a fresh sample
// overwrites both), so no lane that hits pays for their defaults.
template <int MODE, bool LSUM, bool FAST = false, bool ALT = false, bool LEAN = false>
__device__ __forceinline__ bool shade_rec(const rt::TraceParams& P, const Camera& cam, const HitRec& hr, Path& ps,
                                          uint32_t bi, float best, V3& o, V3& d, bool& fresh,
                                          uint32_t* alt = nullptr) {
    static_assert(!LEAN || MODE == rt::MODE_HASH, "camera-batch segments");
    if constexpr (MODE == rt::MODE_PROBE) {   // the closest hit is the answer: no shading, the unit ends
        const size_t i = size_t(ps.px >> 16) * P.band_w + (ps.px & 0xffffu);
        P.probe_out[2 * i] = bi;
        P.probe_out[2 * i + 1] = __float_as_uint(best);
        return false;
    }
    if constexpr (MODE == rt::MODE_FEATURES) {
        // the sample ends at its closest hit: its albedo, oriented normal and depth by the
        // expressions of the shading below, added to the unit's sums; then the unit's next sample
        V3 alb = v3(0.7f, 0.8f, 1.0f), n = v3(0.0f, 0.0f, 0.0f);   // shader.rmiss:15
        float depth = 0.0f, hit = 0.0f;
        if (bi != 0xffffffffu) {
            const V3 p = v3(__builtin_fmaf(best, d.x, o.x), __builtin_fmaf(best, d.y, o.y),
                            __builtin_fmaf(best, d.z, o.z));
            const float4 m0 = hr.m0, m1 = hr.m1;
            const uint32_t ttype = (__float_as_uint(m1.w) >> 8) & 0xffu;
            const V3 outward = normalize(sub(p, v3(hr.g.x, hr.g.y, hr.g.z)));
            const bool front = dot(d, outward) < 0.0f;
            n = front ? outward : neg(outward);
            alb = v3(m0.x, m0.y, m0.z);
            if (ttype == 1u && !checker_positive(p.x, p.y, p.z)) alb = v3(m1.x, m1.y, m1.z);
            depth = best;
            hit = 1.0f;
        }
        FeatPath& fp = feat_path(ps);
        fp.far += alb.x; fp.fag += alb.y; fp.fab += alb.z; fp.fah += hit;
        fp.fnx += n.x; fp.fny += n.y; fp.fnz += n.z; fp.fdz += depth;
        ps.s++;
        if (ps.s >= ps.s_end) return false;
        V3 v;
        camera_ray<rt::MODE_HASH, FAST>(P, cam, ps, o, v);
        d = normalize(v);
        fresh = true;
        return true;
    }
    V3 att;
    bool scatter = false;
    V3 sd, p;
    if constexpr (!LEAN) {
        sd = v3(0.0f, 0.0f, 0.0f);
        p = o;
    }
    UTIL(3, true);
    if (bi == 0xffffffffu) {
        att = v3(0.7f, 0.8f, 1.0f);  // shader.rmiss:15
    } else {
        // shader.rint:33/37 hit attribute; shader.rchit:38-49
        UTIL(10, true);
        if constexpr (LEAN) sd = v3(0.0f, 0.0f, 0.0f);
        p = v3(__builtin_fmaf(best, d.x, o.x), __builtin_fmaf(best, d.y, o.y),
               __builtin_fmaf(best, d.z, o.z));
        const float4 gc4 = hr.g;
        const float4 m0 = hr.m0;
        const float4 m1 = hr.m1;
        const uint32_t tt = __float_as_uint(m1.w);
        const uint32_t mtype = tt & 0xffu, ttype = (tt >> 8) & 0xffu;
        const V3 outward = normalize(sub(p, v3(gc4.x, gc4.y, gc4.z)));
        const bool front = dot(d, outward) < 0.0f;
        const V3 n = front ? outward : neg(outward);
        // shader.rchit:53-64
        att = v3(m0.x, m0.y, m0.z);
        if (ttype == 1u && !checker_positive(p.x, p.y, p.z)) {
            att = v3(m1.x, m1.y, m1.z);
            if constexpr (ALT) *alt = 1u;
        }
        // diffuse and metal both draw one random unit vector first (shader.rchit:69, :80): one
        // copy of that code serves a wave holding both materials
        V3 ru = v3(0.0f, 0.0f, 0.0f);
        if (mtype < 2u) { UTIL(9, true); ru = random_unit_vector(ps.seed); }
        if (mtype == 0u) {                       // diffuse, shader.rchit:68-76
            UTIL(4, true);
            sd = add(n, ru);
            if (fabsf(sd.x) < 1e-8f && fabsf(sd.y) < 1e-8f && fabsf(sd.z) < 1e-8f) sd = n;
        } else if (mtype == 1u) {                // metal, shader.rchit:78-89
            UTIL(5, true);
            const V3 refl = reflect(d, n);
            const V3 fuzz = scale(m0.w, ru);
            const V3 sc = normalize(add(refl, fuzz));
            if (dot(sc, n) > 0.0f) sd = sc;
        } else if (mtype == 2u) {                // dielectric, shader.rchit:91-100,125-133
            UTIL(6, true);
            // eta and r0 = ((1 - eta) / (1 + eta))^2 per face: from the record (solid dielectrics,
            // rt_internal.h make_mat) or computed here (checkered ones: colors[1] is taken)
            float eta, r;
            if (tt & rt::kMatDielConst) {
                eta = front ? m1.x : m0.w;
                r = front ? m1.y : m1.z;
            } else {
                eta = front ? (1.0f / m0.w) : m0.w;
                const float q = (1.0f - eta) / (1.0f + eta);
                r = q * q;
            }
            const float cos_t = dot(neg(d), n);
            bool refracts = false;
            if (eta * sqrt_cr(1.0f - cos_t * cos_t) <= 1.0f) {
                const float refl = r + (1.0f - r) * pow5(1.0f - cos_t);
                refracts = refl < rnd(ps.seed);
            }
            sd = refracts ? refract(d, n, eta) : reflect(d, n);
        }
        scatter = !(sd.x == 0.0f && sd.y == 0.0f && sd.z == 0.0f);  // shader.rchit:48
    }
    if constexpr (MODE == rt::MODE_SCATTER) {   // the bounce itself is the answer: stored, the unit ends
        // Up to and including this branch the MODE_SCATTER path may read nothing of P but probe_out and
        // nothing of cam: rt_scatter_probe_kernel passes a zeroed TraceParams and Camera. (The UTIL
        // points above count into s_util, which that kernel neither clears nor flushes: a -DRT_UTIL
        // build's figures describe the trace kernels only.)
        // case ps.px (rt_scatter_probe_kernel): p, the attenuation, the scatter direction as left
        // above, the direction the next segment is traced along below, does_scatter, the LCG state
        const V3 dn = scatter ? normalize(sd) : v3(0.0f, 0.0f, 0.0f);
        uint32_t* w = P.probe_out + 14u * size_t(ps.px);
        const V3 vs[4] = {p, att, sd, dn};
        for (int k = 0; k < 4; k++) {
            w[3 * k] = __float_as_uint(vs[k].x);
            w[3 * k + 1] = __float_as_uint(vs[k].y);
            w[3 * k + 2] = __float_as_uint(vs[k].z);
        }
        w[12] = scatter ? 1u : 0u;
        w[13] = ps.seed;
        return false;
    }
    // shader.rgen:77-88
    V3 col, v = sd;
    bool more;
    if (scatter) {
        ps.thr = mul(ps.thr, att);
        o = p;
        ps.depth++;
        more = ps.depth < P.max_depth;
        col = mul(ps.thr, v3(0.0f, 0.0f, 0.0f));   // depth exhausted: light stays 0 (Q6)
    } else {
        col = mul(ps.thr, att);
        more = false;
    }
    if (!more) {
        sample_end<MODE, LSUM>(P, ps, col);
        if (ps.s < ps.s_end) {   // the unit's next sample
            camera_ray<MODE, FAST>(P, cam, ps, o, v);
            more = fresh = true;
        }
    }
    if (more) d = normalize(v);
    return more;
}

template <int MODE, bool LSUM>
__device__ __forceinline__ bool shade(const rt::TraceParams& P, const Camera& cam, const float4* __restrict__ geom4,
                                      const float4* __restrict__ mat4, Path& ps, uint32_t bi,
                                      float best, V3& o, V3& d, bool& fresh) {
    HitRec hr{};
    if (bi != 0xffffffffu) hr = load_hit(geom4, mat4, bi);
    return shade_rec<MODE, LSUM>(P, cam, hr, ps, bi, best, o, d, fresh);
}

}  // namespace
