"""The denoiser without a GPU: rt_denoise_check's refusals, the numpy restatement
of the filter (tests/denoise_sim.py) against independent small computations, the restatement's exact
fma against fractions.Fraction, its quality against the oracle's converged frame, and the HIP-free
host half (csrc/rt_denoise_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/native/denoise_host_main.cpp; nothing is loaded into python)."""
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import denoise_sim as ds

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ray-tracing-gpu-vulkan_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
f32 = np.float32


@pytest.fixture(scope="module")
def rtvk():
    import rtvk as m
    m.load_library()
    return m


def test_check_accepts_defaults_and_refuses(rtvk):
    rtvk.denoise_check(None, 1920, 1080, 16)
    rtvk.denoise_check(rtvk.make_denoise(), 1920, 1080, 16)
    d = rtvk.make_denoise()
    assert (d.iterations, d.k_normal, d.k_depth, d.k_color) == ds.DEFAULTS
    for it in range(1, 7):
        rtvk.denoise_check(rtvk.make_denoise(iterations=it), 64, 36, 1)
    rtvk.denoise_check(rtvk.make_denoise(1, 0.0, 0.0, 0.0), 65535, 65535, 256)
    bad = [(rtvk.make_denoise(iterations=0), 64, 36, 16), (rtvk.make_denoise(iterations=7), 64, 36, 16),
           (rtvk.make_denoise(), 64, 36, 0), (rtvk.make_denoise(), 64, 36, 257),
           (rtvk.make_denoise(), 65536, 36, 16), (rtvk.make_denoise(), 64, 65536, 16), (None, 1 << 20, 36, 16)]
    for k in ("k_normal", "k_depth", "k_color"):
        for v in (-1.0, float("inf"), float("-inf"), float("nan")):
            bad.append((rtvk.make_denoise(**{k: v}), 64, 36, 16))
    for params, w, h, f in bad:
        with pytest.raises(rtvk.RtError) as e:
            rtvk.denoise_check(params, w, h, f)
        assert e.value.code == -1 and str(e.value)


def test_fma32_is_the_exact_fma():
    """The restatement's fma (float64 sum rounded to odd) against exact rational arithmetic: random
    operands, cancellations, and sums built to sit on a binary32 tie with a sticky bit beyond
    float64's 53 bits (the case a plain float64 fma double-rounds)."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal(3000).astype(f32) * f32(10.0)
    b = rng.standard_normal(3000).astype(f32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(f32)   # heavy cancellation
    c[::2] = rng.standard_normal(1500).astype(f32) * f32(100.0)
    # ties: a * b = 1 + 2^-11 + 2^-24, the midpoint of two neighbouring binary32 values; c decides
    ta = np.full(4, 1.0 + 2.0 ** -12, f32)
    tb = np.full(4, 1.0 + 2.0 ** -12, f32)
    tc = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -90, -2.0 ** -90], f32)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = ds.fma32(a, b, c)
    want = np.array([ds.fma32_fraction(x, y, z) for x, y, z in zip(a, b, c)], f32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    wrong = int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    print("operands on which a float64 sum double-rounds:", wrong)
    assert wrong >= 2   # the family holds the case the restatement must get right
    assert ds.round_fraction32(Fraction(1) + Fraction(1, 1 << 24)) == f32(1.0)               # tie to even
    assert ds.round_fraction32(Fraction(1) + Fraction(3, 1 << 24)) == f32(1.0 + 2.0 ** -22)  # tie to even, upwards


def test_one_iteration_without_edge_stops_is_the_b3_blur():
    """iterations 1, every k 0: x = 1 and w = K[|dy|] K[|dx|] exactly, the weights of an interior
    texel sum to 1, so e_1 is the 5x5 B3 blur of e_0: against a scalar loop in tap order (bit for
    bit) and against the separable blur in float64."""
    H, W, F, spp = 9, 11, 4, 8
    accum, feat0, feat1 = ds.random_inputs(1, H, W, F)
    mean = ds.denoise(accum, feat0, feat1, F, spp=spp, params=(1, 0.0, 0.0, 0.0))
    e0, a, _, _ = ds.prologue(accum, feat0, feat1, F, spp=spp)
    k1 = np.array([1, 4, 6, 4, 1], np.float64) / 16.0
    for (y, x) in ((2, 2), (4, 5), (6, 8)):
        num = np.zeros(3, f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                num = num + f32(k1[dy + 2] * k1[dx + 2]) * e0[y + dy, x + dx]
        np.testing.assert_array_equal(mean[y, x, :3], num * a[y, x])
        blur = np.einsum("i,j,ijc->c", k1, k1, e0[y - 2:y + 3, x - 2:x + 3].astype(np.float64))
        np.testing.assert_allclose(mean[y, x, :3], blur * a[y, x], rtol=2e-6)
    assert np.all(mean[..., 3] == 1.0)


def test_one_texel_band_returns_its_input():
    accum, feat0, feat1 = ds.random_inputs(2, 1, 1, 3)
    for it in (1, 3, 6):
        mean = ds.denoise(accum, feat0, feat1, 3, spp=5, params=(it, 4.0, 16.0, 1.0))
        c = accum[0, 0, :3] / f32(5.0)
        a = feat0[0, 0, :3] / f32(3.0) + f32(2.0 ** -6)
        np.testing.assert_array_equal(mean[0, 0, :3], (c / a) * a)
    counts = np.zeros((1, 1), np.uint32)
    mean = ds.denoise(accum, feat0, feat1, 3, sample_count=counts)
    np.testing.assert_array_equal(mean[0, 0], f32([0, 0, 0, 1]))


def test_denoised_frame_is_closer_to_the_converged_frame(oracle):
    """Canonical scene, 96x64, 8 spp, 16 feature samples, the default parameters: the restatement's
    PSNR against the oracle's 256-spp frame is strictly above the noisy frame's."""
    W, H, spp, F = 96, 64, 8, 16
    sc = oracle.generate_scene()
    opts = oracle.options(rng_mode=ds.HASH)
    acc, _, _ = oracle.render(sc, oracle.render_call_info(spp, W, H), W, H, opts=opts)
    ref, _, _ = oracle.render(sc, oracle.render_call_info(256, W, H), W, H, opts=opts)
    feat0, feat1 = ds.features(oracle, sc, oracle.render_call_info(spp, W, H), W, H, F)
    mean = ds.denoise(acc, feat0, feat1, F, spp=spp)
    noisy, clean = ds.psnr(acc[..., :3] / f32(spp), ref[..., :3] / f32(256)), ds.psnr(mean, ref[..., :3] / f32(256))
    print(f"PSNR against the 256-spp frame: noisy {noisy:.2f} dB, denoised {clean:.2f} dB")
    assert clean > noisy
    # the features are what they claim: hit fraction in [0, 1], unit-length-or-shorter mean normals
    assert np.all((feat0[..., 3] >= 0) & (feat0[..., 3] <= F))
    assert np.all(np.linalg.norm(feat1[..., :3].astype(np.float64), axis=-1) <= F * (1 + 1e-5))


def test_sky_mask_of_a_one_sample_frame_is_the_feature_miss_mask(oracle):
    """The restated camera rays are the frame's: a 1-spp depth-1 hash frame is the sky colour exactly
    where the features' one sample missed (a low camera, so that the horizon crosses the frame)."""
    W, H = 64, 36
    sc = oracle.generate_scene()
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(np.float32)
    f[8:11] = [13.0, 1.0, 3.0]
    f[12:15] = [-13.0, 0.5, -3.0]
    acc, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(max_depth=1, rng_mode=ds.HASH))
    feat0, _ = ds.features(oracle, sc, rci, W, H, 1)
    sky = np.all(acc[..., :3] == f32(ds.SKY), axis=-1)
    np.testing.assert_array_equal(sky, feat0[..., 3] == 0)
    assert 0.1 < sky.mean() < 0.9


@pytest.mark.timeout(300)
def test_host_half_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "denoise_host_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", *SAN, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "denoise_host_main.cpp"), str(CSRC / "rt_denoise_host.cpp")],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
                            "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "checks passed (ASan + UBSan)" in r.stdout
    assert "runtime error" not in log and "AddressSanitizer" not in log, log[-4000:]
