"""CPU restatement of the first-hit feature buffers and the edge-avoiding denoise
(rt_render_features_device, rt_denoise_device) in binary32 numpy, built on the
unchanged oracle: seeds and random draws from oracle.sample_seed_hash / pixel_seed / random_floats,
winners and t from oracle.closest_hits, the checker's sine from oracle.sinf. The contract's
written-out fmas are restated exactly (fma32: the double sum rounded to odd, then to binary32; the
host tests check it against fractions.Fraction), everything else is one numpy float32 operation per
contract operation. Helper module of test_denoise_host.py, test_gpu_features.py,
test_gpu_denoise.py and test_cli_denoise.py (no tests here)."""
import functools
from fractions import Fraction

import numpy as np

f32 = np.float32
MISS = 0xFFFFFFFF
HASH = 2
SKY = (0.7, 0.8, 1.0)
DEFAULTS = (3, 4.0, 16.0, 1.0)    # iterations, k_normal, k_depth, k_color
KERNEL = (0.375, 0.25, 0.0625)    # B3 spline {6, 4, 1} / 16 by |d|


# ---- exact binary32 fma -----------------------------------------------------------------------

def fma32(a, b, c):
    """round_binary32(a * b + c) for float32 arrays, one rounding. a * b is exact in float64 (48
    bits); the float64 sum s = p + c with its exact error (TwoSum) is rounded to odd (the neighbour
    of s towards the error whose last bit is set, when s is inexact and even): a value rounded to odd
    at 53 bits rounds to nearest at 24 bits as the exact value does, so there is no double rounding."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.atleast_1d(s).view(np.int64) & 1) == 0
    need = (np.atleast_1d(err) != 0) & even & np.isfinite(np.atleast_1d(s))
    toward = np.where(np.atleast_1d(err) > 0, np.inf, -np.inf)
    odd = np.where(need, np.nextafter(np.atleast_1d(s), toward), np.atleast_1d(s))
    return odd.astype(f32).reshape(np.shape(s))


def round_fraction32(x: Fraction) -> np.float32:
    """The binary32 nearest to the rational x (ties to even), by exact comparison."""
    g = f32(float(x))                     # within a few ulp: pick the exact nearest among its neighbours
    cands = [np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))]
    best = None
    for cnd in cands:
        d = abs(Fraction(float(cnd)) - x)
        even = (int(np.array(cnd, f32).view(np.uint32)) & 1) == 0
        key = (d, 0 if even else 1)
        if best is None or key < best[0]:
            best = (key, cnd)
    return f32(best[1])


def fma32_fraction(a, b, c) -> np.float32:
    return round_fraction32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def dot32(a, b):
    """rt_device_math.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def normalize32(v):
    """v * (1 / sqrt(dot(v, v))), both correctly rounded."""
    inv = f32(1.0) / np.sqrt(dot32(v, v))
    return v * inv[..., None]


# ---- camera rays of the counter-based stream --------------------------------------------------

def camera_rays(oracle, rci, W, H, F, rows=None, seed_local=False, sample_base=0):
    """rays [H, W, F, 6] = (o, v): the camera ray of sample sample_base + s of band texel (x, y), as
    rt_render_device traces it under RT_RNG_SAMPLE_HASH (shader.rgen:56-58, 107-115 in binary32;
    the first two draws of the sample's stream are the jitter, the pinhole camera's origin is
    look_from)."""
    r = np.ascontiguousarray(rci, np.uint32)
    number, off_x, off_y, img_w, img_h = int(r[0]), int(r[2]), int(r[3]), int(r[4]), int(r[5])
    vp = np.zeros(18, f32)
    oracle.lib().orc_viewport(r.ctypes.data, vp.ctypes.data)
    look_from, hor, ver, ulc = vp[0:3], vp[3:6], vp[6:9], vp[9:12]
    jit = np.zeros((H, W, F, 2), f32)
    gxy = np.zeros((H, W, 2), f32)
    for y in range(H):
        gy = int(rows[y]) if rows is not None else off_y + y
        for x in range(W):
            gx = off_x + x
            ps = oracle.pixel_seed(x, y, number) if seed_local else oracle.pixel_seed(gx, gy, number)
            gxy[y, x] = (gx, gy)
            for s in range(F):
                jit[y, x, s] = oracle.random_floats(oracle.sample_seed_hash(ps, sample_base + s), 2)
    ux = (gxy[:, :, None, 0] + jit[..., 0]) / f32(img_w)
    uy = (gxy[:, :, None, 1] + jit[..., 1]) / f32(img_h)
    to = (ulc + ux[..., None] * hor) - uy[..., None] * ver
    rays = np.zeros((H, W, F, 6), f32)
    rays[..., 0:3] = look_from
    rays[..., 3:6] = to - look_from
    return rays


# ---- per-sample first-hit values ---------------------------------------------------------------

def sample_values(oracle, scene, rays):
    """[..., 8] float32 per ray: (albedo.rgb, hit, n.xyz, depth) by the expressions of shade_rec."""
    shape = rays.shape[:-1]
    r = np.ascontiguousarray(rays.reshape(-1, 6), f32)
    sc = np.ascontiguousarray(scene, np.uint8).reshape(-1, 80)
    out = np.zeros((r.shape[0], 8), f32)
    out[:, 0:3] = f32(SKY)
    if sc.shape[0]:
        ids, t = oracle.closest_hits(sc, r)
    else:
        ids, t = np.full(r.shape[0], MISS, np.uint32), np.zeros(r.shape[0], f32)
    h = np.flatnonzero(ids != MISS)
    if h.size:
        rec = sc[ids[h]]
        centre = np.ascontiguousarray(rec[:, 0:12]).view(f32).reshape(-1, 3)
        ttype = np.ascontiguousarray(rec[:, 20:24]).view(np.uint32).reshape(-1)
        col = np.ascontiguousarray(rec[:, 32:64]).view(f32).reshape(-1, 2, 4)
        o, v, th = r[h, 0:3], r[h, 3:6], t[h]
        d = normalize32(v)
        p = np.stack([fma32(th, d[:, k], o[:, k]) for k in range(3)], axis=1)
        outward = normalize32(p - centre)
        front = dot32(d, outward) < 0
        n = np.where(front[:, None], outward, -outward)
        alb = col[:, 0, 0:3].copy()
        for i in np.flatnonzero(ttype == 1):      # shader.rchit:58-60: sin(6x) sin(6y) sin(6z) > 0
            sx, sy, sz = (f32(oracle.sinf(float(f32(6.0) * p[i, k]))) for k in range(3))
            if not (sx * sy) * sz > 0:
                alb[i] = col[i, 1, 0:3]
        out[h, 0:3] = alb
        out[h, 3] = 1.0
        out[h, 4:7] = n
        out[h, 7] = th
    return out.reshape(shape + (8,))


def sum_samples(values, F=None):
    """feat0, feat1 [H, W, 4]: the binary32 sums of the first F per-sample values [H, W, S, 8] in
    ascending sample order, starting from the first sample's value."""
    F = values.shape[2] if F is None else F
    acc = values[:, :, 0].copy()
    for s in range(1, F):
        acc = acc + values[:, :, s]
    return np.ascontiguousarray(acc[..., 0:4]), np.ascontiguousarray(acc[..., 4:8])


@functools.lru_cache(maxsize=None)
def _values(oracle, scene_bytes, rci_bytes, W, H, F, rows, seed_local, sample_base):
    scene = np.frombuffer(scene_bytes, np.uint8).reshape(-1, 80)
    rci = np.frombuffer(rci_bytes, np.uint32)
    rays = camera_rays(oracle, rci, W, H, F, None if rows is None else np.array(rows, np.uint32), seed_local,
                       sample_base)
    v = sample_values(oracle, scene, rays)
    v.setflags(write=False)
    return v


def values(oracle, scene, rci, W, H, F, rows=None, seed_local=False, sample_base=0):
    """Per-sample values [H, W, F, 8] of a band, computed once per geometry and shared (read-only)."""
    return _values(oracle, np.ascontiguousarray(scene, np.uint8).tobytes(), np.ascontiguousarray(rci, np.uint32).tobytes(),
                   W, H, F, None if rows is None else tuple(int(r) for r in rows), bool(seed_local), int(sample_base))


def features(oracle, scene, rci, W, H, F, **kw):
    return sum_samples(values(oracle, scene, rci, W, H, F, **kw))


# ---- the filter --------------------------------------------------------------------------------

def prologue(accum, feat0, feat1, F, spp=None, sample_count=None):
    """(e_0 [H, W, 3], a + 2^-6 [H, W, 3], nrm [H, W, 3], z [H, W])."""
    accum, feat0, feat1 = (np.asarray(v, f32) for v in (accum, feat0, feat1))
    H, W = accum.shape[:2]
    n = np.full((H, W), spp, np.uint32) if sample_count is None else np.asarray(sample_count, np.uint32)
    nf = n.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where((n > 0)[..., None], accum[..., 0:3] / nf[..., None], f32(0.0)).astype(f32)
    a = feat0[..., 0:3] / f32(F) + f32(2.0 ** -6)
    nrm = feat1[..., 0:3] / f32(F)
    z = feat1[..., 3] / f32(F)
    return c / a, a, nrm, z


def denoise(accum, feat0, feat1, F, spp=None, sample_count=None, params=DEFAULTS):
    """mean [H, W, 4] float32 = (e_I (a + 2^-6), 1): the contract of include/rt_mi355x.h, every
    operation one float32 numpy operation, taps in order, taps outside the band skipped."""
    iterations, k_normal, k_depth, k_color = params
    k_normal, k_depth, kc = f32(k_normal), f32(k_depth), f32(k_color)
    one = f32(1.0)
    e, a, nrm, z = prologue(accum, feat0, feat1, F, spp, sample_count)
    H, W = z.shape
    for i in range(iterations):
        step = 1 << i
        num = np.zeros((H, W, 3), f32)
        den = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                dn = nrm[P] - nrm[Q]
                dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                dz = (z[P] - z[Q]) / (z[P] + one)
                de = e[P] - e[Q]
                de2 = (de[..., 0] * de[..., 0] + de[..., 1] * de[..., 1]) + de[..., 2] * de[..., 2]
                x = ((one + k_normal * dn2) * (one + k_depth * (dz * dz))) * (one + kc * de2)
                w = (f32(KERNEL[abs(dy)]) * f32(KERNEL[abs(dx)])) / (x * x)
                num[P] = num[P] + w[..., None] * e[Q]
                den[P] = den[P] + w
        e = num / den[..., None]
        kc = kc * f32(4.0)
    mean = np.ones((H, W, 4), f32)
    mean[..., 0:3] = e * a
    assert mean.dtype == f32 and e.dtype == f32
    return mean


def random_inputs(seed, H, W, F):
    """(accum, feat0, feat1) [H, W, 4] float32 of a seeded generator: finite sums of no scene, so that a
    check on them does not depend on an image's smoothness (albedo sums in [0, F], normal sums in
    [-F, F], depth sums in [0, 30 F], colour sums in [0, 8))."""
    rng = np.random.default_rng(seed)
    accum = np.ones((H, W, 4), f32)
    accum[..., :3] = rng.uniform(0.0, 8.0, (H, W, 3))
    feat0 = rng.uniform(0.0, F, (H, W, 4)).astype(f32)
    feat1 = rng.uniform(-F, F, (H, W, 4)).astype(f32)
    feat1[..., 3] = rng.uniform(0.0, 30.0 * F, (H, W))
    return accum, feat0, feat1


def psnr(mean, ref_mean):
    """PSNR (dB) of sqrt(clip(mean)) against sqrt(clip(ref_mean)), both [H, W, >= 3] linear means."""
    a = np.sqrt(np.clip(np.asarray(mean, np.float64)[..., 0:3], 0.0, 1.0))
    b = np.sqrt(np.clip(np.asarray(ref_mean, np.float64)[..., 0:3], 0.0, 1.0))
    return float(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))
