"""The motion pass without a GPU: rt_motion_check's accept and refuse cases through
rtvk, the numpy restatement (tests/motion_sim.py) against an independent scalar loop on a few texels,
the properties the reprojected call builds on (a frame against itself lands on its own texel centres
far inside the snap, a camera shifted by one pixel's width moves a plane by one texel, a texel behind
the previous camera and a changed sphere count are not ok), and the HIP-free host half
(csrc/rt_motion_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/native/motion_host_main.cpp; nothing is loaded into python)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_sim as ds
import motion_sim as ms

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ray-tracing-gpu-vulkan_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
f32 = np.float32
SNAP = 2.0 ** -6


@pytest.fixture(scope="module")
def rtvk():
    import rtvk as m
    m.load_library()
    return m


def moved_camera(oracle, spp, W, H, s, k, **kw):
    """Frame k's RenderCallInfo on the path of DESIGN.md §3.1.3: the camera at (13 + s k, 11, -3 + 2 s k),
    looking at the origin."""
    rci = oracle.render_call_info(spp, W, H, **kw)
    f = rci.view(f32)
    pos = f32([13.0, 11.0, -3.0]) + f32(k) * f32([s, 0.0, 2.0 * s])
    f[8:11] = pos
    f[12:15] = -pos
    return rci


def test_check_accepts_and_refuses(rtvk, oracle):
    mk = lambda w, h: rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(1, w, h).tobytes())
    rtvk.motion_check(1920, 1080, mk(1920, 1080))
    rtvk.motion_check(37, 19, mk(64, 36), mk(64, 36))
    rtvk.motion_check(65535, 65535, mk(8, 8))
    bad = [(65536, 36, mk(64, 36), None, "width"), (64, 65536, mk(64, 36), None, "height"),
           (64, 36, None, None, "rci"), (64, 36, mk(0, 36), None, "image_size"), (64, 36, mk(64, 0), None, "image_size"),
           (64, 36, mk(64, 36), mk(64, 37), "previous"), (64, 36, mk(64, 36), mk(96, 36), "previous")]
    for w, h, rci, prev, field in bad:
        with pytest.raises(rtvk.RtError) as e:
            rtvk.motion_check(w, h, rci, prev)
        assert e.value.code == -1 and field in str(e.value), (field, str(e.value))


# ---- the restatement against a scalar loop --------------------------------------------------------

def fma(a, b, c):
    return ds.fma32_fraction(f32(a), f32(b), f32(c))


def dot(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], f32(a[0]) * f32(b[0])))


def scalar_motion(oracle, scene, rci, prev_scene, prev_rci, x, y):
    """(sx, sy, dzm, ok) of band texel (x, y), one float32 operation at a time, fmas by exact rationals."""
    r = np.ascontiguousarray(rci, np.uint32)
    off_x, off_y, img_w, img_h = int(r[2]), int(r[3]), int(r[4]), int(r[5])
    lf, hor, ver, ulc = ms.viewport(oracle, rci)
    ux = f32(np.float64(f32(off_x + x) + f32(0.5)) * (1.0 / np.float64(img_w)))
    uy = f32(np.float64(f32(off_y + y) + f32(0.5)) * (1.0 / np.float64(img_h)))
    v = [f32(f32(f32(ulc[c] + f32(ux * hor[c])) - f32(uy * ver[c])) - lf[c]) for c in range(3)]
    inv = f32(1.0) / np.sqrt(dot(v, v))
    d = [f32(v[c] * inv) for c in range(3)]
    ids, t = oracle.closest_hits(scene, np.array([list(lf) + v], f32)) if len(scene) else ([ds.MISS], [f32(0)])
    hit, t = int(ids[0]) != ds.MISS, f32(t[0])
    lfp, horp, verp, ulcp = ms.viewport(oracle, prev_rci)
    same = len(scene) == len(prev_scene) and len(scene) > 0
    if hit:
        p = [fma(t, d[c], lf[c]) for c in range(3)]
        if same:
            cn, cp = ms.centres(scene)[int(ids[0])], ms.centres(prev_scene)[int(ids[0])]
            p = [f32(f32(p[c] - cn[c]) + cp[c]) for c in range(3)]
        rr = [f32(p[c] - lfp[c]) for c in range(3)]
    else:
        rr = d
    u = [f32(ulcp[c] - lfp[c]) for c in range(3)]
    wn = [f32(f32(horp[1] * verp[2]) - f32(horp[2] * verp[1])), f32(f32(horp[2] * verp[0]) - f32(horp[0] * verp[2])),
          f32(f32(horp[0] * verp[1]) - f32(horp[1] * verp[0]))]
    with np.errstate(all="ignore"):
        den = dot(rr, wn)
        s = f32(dot(u, wn) / den)
        rel = [f32(f32(s * rr[c]) - u[c]) for c in range(3)]
        sx = f32(f32(f32(dot(rel, horp) * f32(f32(1.0) / dot(horp, horp))) * f32(img_w)) - f32(off_x))
        sy = f32(f32(-f32(dot(rel, verp) * f32(f32(1.0) / dot(verp, verp))) * f32(img_h)) - f32(off_y))
        dzm = f32(np.sqrt(dot(rr, rr)) - t) if hit else f32(0.0)
    ok = bool(den > 0 and np.isfinite(sx) and np.isfinite(sy) and (not hit or same))
    return np.array([sx, sy, dzm, f32(1.0 if ok else 0.0)], f32)


def test_fma32_is_exact():
    rng = np.random.default_rng(2)
    a, b, c = (rng.normal(size=200).astype(f32) for _ in range(3))
    c[:50] = -(a[:50] * b[:50])           # cancellation
    got = ds.fma32(a, b, c)
    for i in range(200):
        assert got[i] == ds.fma32_fraction(a[i], b[i], c[i])


def test_restatement_equals_the_scalar_loop(oracle):
    """A 37 x 19 band at offset (9, 5) of a 64 x 36 image, the scene at t = 0 against t = 0.2 with the
    camera at frame 1 of the s = 0.2 path against frame 0: hits of moving and static spheres, the
    ground and the sky."""
    W, H = 37, 19
    sc, prev = oracle.generate_scene(0.0), oracle.generate_scene(0.2)
    rci = moved_camera(oracle, 1, 64, 36, 0.2, 1, offset=(9, 5))
    prev_rci = moved_camera(oracle, 1, 64, 36, 0.2, 0, offset=(9, 5))
    got = ms.motion(oracle, sc, rci, W, H, prev, prev_rci)
    assert got.dtype == f32 and got.shape == (H, W, 4)
    for x, y in ((0, 0), (36, 18), (18, 9), (5, 14), (30, 3), (20, 12), (11, 7)):
        want = scalar_motion(oracle, sc, rci, prev, prev_rci, x, y)
        np.testing.assert_array_equal(got[y, x].view(np.uint32), want.view(np.uint32), err_msg=str((x, y)))
    assert np.all(got[..., 3] == 1) and np.abs(got[..., 0] - (np.arange(W) + 0.5)).max() > 0.25


# ---- what the reprojected call builds on -----------------------------------------------------------

def test_a_frame_against_itself_lands_inside_the_snap(oracle):
    """No previous frame: every texel of a 96 x 54 frame of the canonical scene gets its own centre back
    to within 2^-6 of a texel, and no distance changed by more than rounding."""
    W, H = 96, 54
    m = ms.motion(oracle, oracle.generate_scene(0.0), oracle.render_call_info(1, W, H), W, H)
    ex = np.abs(m[..., 0].astype(np.float64) - (np.arange(W) + 0.5)[None, :])
    ey = np.abs(m[..., 1].astype(np.float64) - (np.arange(H) + 0.5)[:, None])
    print(f"a frame against itself at {W}x{H}: max |sx - (x + 0.5)| {ex.max():.3g}, max |sy - (y + 0.5)| {ey.max():.3g}, "
          f"max |dzm| {np.abs(m[..., 2]).max():.3g}")
    assert ex.max() < SNAP and ey.max() < SNAP
    assert np.all(m[..., 3] == 1) and np.abs(m[..., 2]).max() < 1e-2
    # the same on an offset band of a larger image, and with the moved camera
    rci = moved_camera(oracle, 1, 64, 36, 0.2, 3, offset=(9, 5))
    m = ms.motion(oracle, oracle.generate_scene(0.6), rci, 37, 19)
    assert np.abs(m[..., 0] - (np.arange(37) + 0.5)[None, :]).max() < SNAP
    assert np.abs(m[..., 1] - (np.arange(19) + 0.5)[:, None]).max() < SNAP


def plane_scene(oracle, rci):
    """One sphere of radius 1000 that touches the camera's focus plane on the optical axis: inside the
    view its surface leaves that plane by less than 1e-3 of its distance."""
    lf, hor, ver, ulc = ms.viewport(oracle, rci)
    fwd = np.cross(hor.astype(np.float64), ver.astype(np.float64))
    fwd /= np.linalg.norm(fwd)
    sc = oracle.generate_scene(0.0)[:1].copy()
    geo = np.append(lf.astype(np.float64) + 1010.0 * fwd, 1000.0).astype(f32)
    sc[0, 0:16] = geo.view(np.uint8)
    return sc, hor


def test_a_camera_shifted_by_one_pixel_moves_a_plane_by_one_texel(oracle):
    W, H = 96, 54
    rci = oracle.render_call_info(1, W, H)
    sc, hor = plane_scene(oracle, rci)
    prev_rci = rci.copy()
    prev_rci.view(f32)[8:11] += hor / f32(W)      # the same direction: a pure translation along hor
    m = ms.motion(oracle, sc, rci, W, H, sc, prev_rci)
    assert np.all(m[..., 3] == 1)
    ex = np.abs(m[..., 0].astype(np.float64) - (np.arange(W) - 0.5)[None, :])
    ey = np.abs(m[..., 1].astype(np.float64) - (np.arange(H) + 0.5)[:, None])
    print(f"one pixel along hor: max |sx - (x - 0.5)| {ex.max():.3g}, max |sy - (y + 0.5)| {ey.max():.3g}")
    assert ex.max() < SNAP and ey.max() < SNAP


def test_a_texel_behind_the_previous_camera_is_not_ok(oracle):
    W, H = 40, 24
    sc = oracle.generate_scene(0.0)
    rci = oracle.render_call_info(1, W, H)
    prev_rci = rci.copy()
    prev_rci.view(f32)[12:15] *= f32(-1.0)       # the previous camera looked the other way
    m = ms.motion(oracle, sc, rci, W, H, sc, prev_rci)
    assert np.all(m[..., 3] == 0)
    ahead = ms.motion(oracle, sc, rci, W, H, sc, rci)
    assert np.all(ahead[..., 3] == 1)


def test_a_changed_sphere_count_invalidates_hits_and_keeps_the_sky(oracle):
    W, H = 40, 24
    sc = oracle.generate_scene(0.0)
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(f32)
    f[8:11] = [13.0, 1.0, 3.0]                   # low: the horizon crosses the frame
    f[12:15] = [-13.0, 0.5, -3.0]
    rays = ms.centre_rays(oracle, rci, W, H)
    ids, _ = ms.hits(oracle, sc, rays)
    hit = ids != ds.MISS
    assert 0.1 < hit.mean() < 0.9
    m = ms.motion(oracle, sc, rci, W, H, sc[:-1], rci)
    assert np.all(m[..., 3][hit] == 0) and np.all(m[..., 3][~hit] == 1)
    assert np.abs(m[..., 0] - (np.arange(W) + 0.5)[None, :])[~hit].max() < SNAP and np.all(m[..., 2][~hit] == 0)
    same = ms.motion(oracle, sc, rci, W, H, sc, rci)
    assert np.all(same[..., 3] == 1)


@pytest.mark.timeout(300)
def test_host_half_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "motion_host_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", *SAN, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "motion_host_main.cpp"), str(CSRC / "rt_motion_host.cpp"),
                        str(CSRC / "rt_denoise_host.cpp")],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
                            "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "checks passed (ASan + UBSan)" in r.stdout
    assert "runtime error" not in log and "AddressSanitizer" not in log, log[-4000:]
