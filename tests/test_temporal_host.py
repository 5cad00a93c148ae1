"""The temporal stage without a GPU: rt_temporal_check's accept and refuse cases
through rtvk, the numpy restatement (tests/temporal_sim.py) against independent scalar loops on
denoise_sim.random_inputs, and the HIP-free host half (csrc/rt_temporal_host.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/native/temporal_host_main.cpp; nothing is loaded into python)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import temporal_sim as ts

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
    rtvk.temporal_check(None, 1920, 1080, 16)
    rtvk.temporal_check(rtvk.make_temporal(), 1920, 1080, 16)
    d = rtvk.make_temporal()
    assert (d.max_history, d.k_normal, d.k_depth) == ts.DEFAULTS and d.reserved == 0
    mk = rtvk.make_temporal
    for n in (2, 65535):
        rtvk.temporal_check(mk(max_history=n), 64, 36, 1)
    rtvk.temporal_check(mk(2, 0.0, 0.0), 65535, 65535, 256)
    res = mk()
    res.reserved = 1
    bad = [(mk(max_history=0), 64, 36, 16, "max_history"), (mk(max_history=1), 64, 36, 16, "max_history"),
           (mk(max_history=65536), 64, 36, 16, "max_history"), (res, 64, 36, 16, "reserved"),
           (mk(), 64, 36, 0, "feature_samples"), (mk(), 64, 36, 257, "feature_samples"),
           (mk(), 65536, 36, 16, "width"), (mk(), 64, 65536, 16, "height"), (None, 65536, 36, 16, "width")]
    for k in ("k_normal", "k_depth"):
        for v in (-1.0, float("inf"), float("nan")):
            bad.append((mk(**{k: v}), 64, 36, 16, k))
    for params, w, h, f, field in bad:
        with pytest.raises(rtvk.RtError) as e:
            rtvk.temporal_check(params, w, h, f)
        assert e.value.code == -1 and field in str(e.value), (field, str(e.value))


# ---- the restatement against scalar loops ---------------------------------------------------------

def scalar_e(accum, feat0, F, h, y, x):
    """e = (A.rgb / h) / (feat0.rgb / F + 2^-6) of one texel, one float32 operation at a time."""
    return np.array([(f32(accum[y, x, c]) / f32(h)) / (f32(feat0[y, x, c]) / f32(F) + f32(2.0 ** -6)) for c in range(3)], f32)


def scalar_a(feat0, F, y, x):
    return np.array([f32(feat0[y, x, c]) / f32(F) + f32(2.0 ** -6) for c in range(3)], f32)


def test_frame_zero_is_the_frame_itself():
    """An empty history: out = (c / a) a, n = 1, the guide is the frame's; two accumulators alike and
    the mean is ((eA + eB) 0.5) a."""
    H, W, F, h = 5, 7, 4, 3
    A, feat0, feat1 = ts.random_inputs(3, H, W, F)
    B, _, _ = ts.random_inputs(4, H, W, F)
    st = ts.State(H, W)
    out_a, out_b, mean, n = ts.accumulate(st, A, feat0, feat1, F, accum_b=B, spp=h)
    assert np.all(n == 1) and np.all(st.ha[..., 3] == 1) and np.all(st.hb[..., 3] == 1)
    for y in range(H):
        for x in range(W):
            ea, eb, a = scalar_e(A, feat0, F, h, y, x), scalar_e(B, feat0, F, h, y, x), scalar_a(feat0, F, y, x)
            np.testing.assert_array_equal(out_a[y, x], np.append(ea * a, f32(1)))
            np.testing.assert_array_equal(out_b[y, x], np.append(eb * a, f32(1)))
            np.testing.assert_array_equal(mean[y, x, :3], ((ea + eb) * f32(0.5)) * a)
            np.testing.assert_array_equal(st.ha[y, x, :3], ea)
            np.testing.assert_array_equal(st.hg[y, x], feat1[y, x] / f32(F))
    st1 = ts.State(H, W)
    one_a, none_b, mean1, _ = ts.accumulate(st1, A, feat0, feat1, F, spp=h)
    assert none_b is None and np.all(st1.hb == 0)
    np.testing.assert_array_equal(one_a, out_a)
    np.testing.assert_array_equal(mean1, one_a)


def test_the_same_inputs_again_change_no_bit():
    """A static scene with repeated noise: x = 1 exactly, every texel valid, HA + alpha (e - HA) = HA:
    the frame-0 output bit for bit, and n = min(m, N)."""
    H, W, F, N = 6, 9, 5, 3
    A, feat0, feat1 = ts.random_inputs(11, H, W, F)
    B, _, _ = ts.random_inputs(12, H, W, F)
    st = ts.State(H, W)
    first = None
    for m in range(1, 7):
        out = ts.accumulate(st, A, feat0, feat1, F, accum_b=B, spp=2, params=(N, 4.0, 16.0))
        first = first or out
        for got, want in zip(out[:3], first[:3]):
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.all(out[3] == min(m, N))


def test_running_mean_then_exponential_average():
    """Equal guides, different colours: e' is the running mean of the first N frames (1e-5 relative),
    afterwards the exponential average of weight 1 / N."""
    H, W, F, N, frames = 4, 5, 4, 4, 9
    _, feat0, feat1 = ts.random_inputs(21, H, W, F)
    st = ts.State(H, W)
    a = (feat0[..., :3] / f32(F) + f32(2.0 ** -6)).astype(np.float64)
    es, want = [], None
    for k in range(frames):
        A, _, _ = ts.random_inputs(100 + k, H, W, F)
        e = A[..., :3].astype(np.float64) / 2.0 / a
        es.append(e)
        _, _, _, n = ts.accumulate(st, A, feat0, feat1, F, spp=2, params=(N, 4.0, 16.0))
        assert np.all(n == min(k + 1, N))
        if k < N:
            want = np.mean(es, axis=0)
        else:
            want = want + (e - want) / N
        np.testing.assert_allclose(st.ha[..., :3], want, rtol=1e-5)


def test_a_flipped_normal_resets_its_texel_alone():
    """A texel whose normal sum is negated between frames starts over from the current frame (dn2 = 4
    |nrm|^2, far above the stop); so does one whose depth doubles; their neighbours integrate."""
    H, W, F = 5, 6, 4
    A0, feat0, feat1 = ts.random_inputs(31, H, W, F)
    feat1[..., :3] = np.where(np.abs(feat1[..., :3]) < 1.0, f32(2.0), feat1[..., :3])   # no normal near 0
    feat1[..., 3] = np.maximum(feat1[..., 3], f32(F))                                    # z >= 1
    A1, _, _ = ts.random_inputs(32, H, W, F)
    st = ts.State(H, W)
    ts.accumulate(st, A0, feat0, feat1, F, spp=2)
    before = st.copy()
    g1 = feat1.copy()
    g1[2, 3, :3] = -g1[2, 3, :3]
    g1[1, 1, 3] = g1[1, 1, 3] * f32(2.0)
    out_a, _, _, n = ts.accumulate(st, A1, feat0, g1, F, spp=2)
    for y in range(H):
        for x in range(W):
            e1, a = scalar_e(A1, feat0, F, 2, y, x), scalar_a(feat0, F, y, x)
            if (y, x) in ((2, 3), (1, 1)):
                assert n[y, x] == 1
                np.testing.assert_array_equal(st.ha[y, x, :3], e1)
                np.testing.assert_array_equal(out_a[y, x, :3], e1 * a)
            else:
                assert n[y, x] == 2
                hist = before.ha[y, x, :3]
                np.testing.assert_array_equal(st.ha[y, x, :3], hist + (f32(1.0) / f32(2.0)) * (e1 - hist))
            np.testing.assert_array_equal(st.hg[y, x], g1[y, x] / f32(F))


def test_no_measurement_keeps_a_valid_history_and_zeroes_an_invalid_one():
    H, W, F = 4, 4, 4
    A0, feat0, feat1 = ts.random_inputs(41, H, W, F)
    feat1[..., :3] = np.where(np.abs(feat1[..., :3]) < 1.0, f32(2.0), feat1[..., :3])
    A1, _, _ = ts.random_inputs(42, H, W, F)
    st = ts.State(H, W)
    ts.accumulate(st, A0, feat0, feat1, F, spp=2)
    ts.accumulate(st, A0, feat0, feat1, F, spp=2)
    before = st.copy()
    counts = np.full((H, W), 2, np.uint32)
    counts[0, 0] = counts[3, 2] = counts[1, 1] = 0
    g1 = feat1.copy()
    g1[1, 1, :3] = -g1[1, 1, :3]                       # no samples and no valid history
    out_a, _, _, n = ts.accumulate(st, A1, feat0, g1, F, sample_count=counts)
    for (y, x) in ((0, 0), (3, 2)):
        assert n[y, x] == 2
        np.testing.assert_array_equal(st.ha[y, x], before.ha[y, x])
        np.testing.assert_array_equal(out_a[y, x, :3], before.ha[y, x, :3] * scalar_a(feat0, F, y, x))
    assert n[1, 1] == 0 and np.all(st.ha[1, 1] == 0) and np.all(out_a[1, 1] == f32([0, 0, 0, 1]))
    np.testing.assert_array_equal(st.hg[1, 1], g1[1, 1] / f32(F))
    assert n[2, 2] == 3
    # an empty history and no samples: black, n = 0; the next measured frame is a first frame
    st2 = ts.State(H, W)
    out_a, _, _, n = ts.accumulate(st2, A1, feat0, feat1, F, sample_count=np.zeros((H, W), np.uint32))
    assert np.all(n == 0) and np.all(out_a[..., :3] == 0) and np.all(st2.ha == 0)
    _, _, _, n = ts.accumulate(st2, A1, feat0, feat1, F, spp=2)
    assert np.all(n == 1)


@pytest.mark.timeout(300)
def test_host_half_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "temporal_host_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", *SAN, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "temporal_host_main.cpp"), str(CSRC / "rt_temporal_host.cpp"),
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
