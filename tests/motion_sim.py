"""CPU restatement of the motion pass (rt_render_motion_device; include/rt_mi355x.h)
in binary32 numpy, built on the unchanged oracle: the cameras from oracle's orc_viewport, winners and t
from oracle.closest_hits, the contract's written-out fmas by denoise_sim.fma32 / dot32 / normalize32,
everything else one float32 numpy operation per contract operation, in the contract's order. Helper
module of test_motion_host.py, test_gpu_motion.py, test_gpu_temporal_reproject.py,
test_cli_reproject.py and test_temporal_reproject_quality.py (no tests here)."""
import numpy as np

from denoise_sim import MISS, dot32, fma32, normalize32

f32 = np.float32


def viewport(oracle, rci):
    """(look_from, hor, ver, ulc), float32 [3] each, of a RenderCallInfo."""
    r = np.ascontiguousarray(rci, np.uint32)
    vp = np.zeros(18, f32)
    oracle.lib().orc_viewport(r.ctypes.data, vp.ctypes.data)
    return vp[0:3].copy(), vp[3:6].copy(), vp[6:9].copy(), vp[9:12].copy()


def cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def projection(oracle, prev_rci):
    """The launch constants of the previous camera: (lf', hor', ver', u, wn, k, ihh, ivv)."""
    lf, hor, ver, ulc = viewport(oracle, prev_rci)
    u = ulc - lf
    wn = cross32(hor, ver)
    k = dot32(u, wn)
    ihh = f32(1.0) / dot32(hor, hor)
    ivv = f32(1.0) / dot32(ver, ver)
    assert all(v.dtype == f32 for v in (u, wn, k, ihh, ivv))
    return lf, hor, ver, u, wn, k, ihh, ivv


def centre_rays(oracle, rci, W, H):
    """rays [H, W, 6] = (o, v) through the centres of the band's texels: camera_ray without jitter."""
    r = np.ascontiguousarray(rci, np.uint32)
    off_x, off_y, img_w, img_h = int(r[2]), int(r[3]), int(r[4]), int(r[5])
    lf, hor, ver, ulc = viewport(oracle, rci)
    gx = (np.arange(W, dtype=np.uint32) + np.uint32(off_x)).astype(f32) + f32(0.5)
    gy = (np.arange(H, dtype=np.uint32) + np.uint32(off_y)).astype(f32) + f32(0.5)
    ux = (gx.astype(np.float64) * (1.0 / np.float64(f32(img_w)))).astype(f32)
    uy = (gy.astype(np.float64) * (1.0 / np.float64(f32(img_h)))).astype(f32)
    to = (ulc + ux[None, :, None] * hor) - uy[:, None, None] * ver
    rays = np.zeros((H, W, 6), f32)
    rays[..., 0:3] = lf
    rays[..., 3:6] = to - lf
    assert to.dtype == f32
    return rays


def hits(oracle, scene, rays):
    """(ids uint32, t float32) of rays [..., 6], the rays' shape without the last axis."""
    shape = rays.shape[:-1]
    r = np.ascontiguousarray(rays.reshape(-1, 6), f32)
    sc = np.ascontiguousarray(scene, np.uint8).reshape(-1, 80)
    if sc.shape[0]:
        ids, t = oracle.closest_hits(sc, r)
    else:
        ids, t = np.full(r.shape[0], MISS, np.uint32), np.zeros(r.shape[0], f32)
    return ids.reshape(shape), t.reshape(shape)


def centres(scene):
    sc = np.ascontiguousarray(scene, np.uint8).reshape(-1, 80)
    return np.ascontiguousarray(sc[:, 0:12]).view(f32).reshape(-1, 3)


def motion_from_hits(oracle, rays, ids, t, scene, rci, prev_scene=None, prev_rci=None):
    """The third launch: motion [..., 4] = (sx, sy, dzm, ok) from the rays and their (id, t)."""
    r_ = np.ascontiguousarray(rci, np.uint32)
    off_x, off_y, img_w, img_h = f32(int(r_[2])), f32(int(r_[3])), f32(int(r_[4])), f32(int(r_[5]))
    prev_rci = rci if prev_rci is None else prev_rci
    prev_scene = scene if prev_scene is None else prev_scene
    lf, hor, ver, u, wn, k, ihh, ivv = projection(oracle, prev_rci)
    c_now, c_prev = centres(scene), centres(prev_scene)
    same = c_now.shape[0] == c_prev.shape[0] and c_now.shape[0] > 0
    o, v = rays[..., 0:3], rays[..., 3:6]
    d = normalize32(v)
    hit = ids != MISS
    safe = np.where(hit, ids, 0).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p = np.stack([fma32(t, d[..., c], o[..., c]) for c in range(3)], axis=-1)
        if same:
            p = (p - c_now[safe]) + c_prev[safe]
        r = np.where(hit[..., None], p - lf, d).astype(f32)
        den = dot32(r, np.broadcast_to(wn, r.shape))
        s = k / den
        rel = s[..., None] * r - u
        sx = ((dot32(rel, np.broadcast_to(hor, r.shape)) * ihh) * img_w) - off_x
        sy = ((-(dot32(rel, np.broadcast_to(ver, r.shape)) * ivv)) * img_h) - off_y
        dzm = np.where(hit, np.sqrt(dot32(r, r)) - t, f32(0.0)).astype(f32)
    ok = (den > 0) & np.isfinite(sx) & np.isfinite(sy) & (~hit | same)
    out = np.stack([sx, sy, dzm, ok.astype(f32)], axis=-1)
    assert out.dtype == f32 and rel.dtype == f32 and s.dtype == f32
    return out


def motion(oracle, scene, rci, W, H, prev_scene=None, prev_rci=None):
    """The motion plane [H, W, 4] of a band: the three launches."""
    rays = centre_rays(oracle, rci, W, H)
    ids, t = hits(oracle, scene, rays)
    return motion_from_hits(oracle, rays, ids, t, scene, rci, prev_scene, prev_rci)
