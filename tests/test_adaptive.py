"""Adaptive frames (rt_render_adaptive_device): the stop criterion against Python
ints on the CPU, and on the GPU every texel of an adaptive frame against the unchanged oracle.

The counter-based stream makes the reference exact: sample s of a pixel is a pure function of
(pixel_seed, s) and sums are integers, so a pixel whose tile stopped at n samples holds bit for bit
what oracle.render(spp=n) gives, and the pass loop simulated on the oracle's per-sample cube
(adaptive_sim.py) predicts the count map exactly.
"""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402

HASH = 2
BRUTE, AUTO = 1, 0
MIN, STEP, MAX, THR = 8, 8, 64, 0.2
THR_Q16 = 13107


@pytest.fixture(scope="module")
def lib(oracle):
    import rtvk
    return rtvk


# ---- CPU: the criterion and the binding ---------------------------------------------------------
def _check(lib, E, S, n, m, thr):
    assert lib.adaptive_tile_converged(E, S, n, m, thr) == sim.converged(E, S, n, m, thr), (E, S, n, m, thr)


@pytest.mark.parametrize("thr", [1, 13107, 65535, (1 << 20) - 1])
@pytest.mark.parametrize("m", [1, 27, 64])
def test_criterion_at_the_boundary(lib, thr, m):
    """2^17 E equal to thr S', one below and one above it (thr odd, so thr S' = +-1 mod 2^17 has a
    solution): equality and above are not converged, the strict inequality is."""
    n = 8
    guard = n * 3 * m << 16
    inv = pow(thr, -1, 1 << 17)
    for j in (1, 12345, (1 << 28) + 77):
        # equality: S' a multiple of 2^17 beyond the guard
        s1 = ((guard >> 17) + j) << 17
        E = thr * (s1 >> 17)
        assert (E << 17) == thr * s1
        assert lib.adaptive_tile_converged(E, s1 - guard, n, m, thr) is False
        _check(lib, E, s1 - guard, n, m, thr)
        # thr S' = 2^17 E + 1: converged
        s1 = ((guard >> 17) + j << 17) + inv
        assert (thr * s1 - 1) % (1 << 17) == 0
        E = (thr * s1 - 1) >> 17
        assert lib.adaptive_tile_converged(E, s1 - guard, n, m, thr) is True
        _check(lib, E, s1 - guard, n, m, thr)
        # thr S' = 2^17 E - 1: not converged
        s1 = ((guard >> 17) + j << 17) + ((1 << 17) - inv)
        assert (thr * s1 + 1) % (1 << 17) == 0
        E = (thr * s1 + 1) >> 17
        assert lib.adaptive_tile_converged(E, s1 - guard, n, m, thr) is False
        _check(lib, E, s1 - guard, n, m, thr)


def test_criterion_thresholds_and_large_sums(lib):
    big = (1 << 50) - 1
    for m in (1, 27, 64):
        for n in (2, 64, 1 << 19):
            for thr in (0, 1, 13107, 1 << 20):
                for E, S in ((0, 0), (big, big), (big, 1 << 50), (big - 5, (1 << 51) - 3), (1, 0), (0, 1),
                             (big, 0), ((1 << 33) + 1, (1 << 47) + 12345)):
                    _check(lib, E, S, n, m, thr)
            # threshold 0 never converges, threshold 16 always does (E <= S)
            assert lib.adaptive_tile_converged(0, 0, n, m, 0) is False
            assert lib.adaptive_tile_converged(big, big, n, m, 1 << 20) is True


def test_criterion_random(lib):
    rnd = random.Random(20240611)
    for _ in range(4000):
        bits = rnd.randrange(1, 51)
        S = rnd.randrange(1 << bits)
        E = rnd.randrange(S + 1) if rnd.random() < 0.8 else rnd.randrange(1 << 50)
        n = 2 * rnd.randrange(1, (1 << 18) + 1)
        m = rnd.choice((1, 27, 64, rnd.randrange(1, 65)))
        thr = rnd.choice((0, 1, 13107, 1 << 20, rnd.randrange(1 << 21)))
        if rnd.random() < 0.3 and thr:   # near the boundary
            E = min((1 << 50), max(0, thr * (S + (n * 3 * m << 16)) // (1 << 17) + rnd.randrange(-1, 2)))
        _check(lib, E, S, n, m, thr)


def test_criterion_refuses_out_of_range(lib):
    from rtvk import RtError
    for args in ((1 << 56, 0, 8, 64, 1), (0, 1 << 56, 8, 64, 1), (0, 0, (1 << 19) + 1, 64, 1), (0, 0, 8, 0, 1),
                 (0, 0, 8, 65, 1)):
        with pytest.raises(RtError):
            lib.adaptive_tile_converged(*args)


def test_binding_layout_and_threshold_rounding(lib):
    from rtvk import abi
    assert ctypes.sizeof(abi.Adaptive) == 16 and ctypes.sizeof(abi.AdaptiveInfo) == 24
    assert abi.AdaptiveInfo.samples.offset == 16 and abi.Adaptive.threshold.offset == 8
    a = lib.make_adaptive(0.2, 8, 16)
    assert (a.min_spp, a.step_spp, a.reserved) == (8, 16, 0) and a.threshold == np.float32(0.2)
    assert lib.threshold_q16(0.2) == 13107 and lib.threshold_q16(0.0) == 0 and lib.threshold_q16(16.0) == 1 << 20
    # floor(x * 65536 + 0.5) of the binary32 value: halves round up
    assert lib.threshold_q16(1.5 / 65536) == 2 and lib.threshold_q16(0.49 / 65536) == 0
    assert lib.threshold_q16(THR) == THR_Q16


# ---- GPU ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def renderer(lib, torch):
    r = lib.Renderer(0)
    yield r
    r.close()


def gpu_adaptive(lib, renderer, torch, oracle, W, H, k=11, accel=AUTO, rows=None, base=0, image=None, thr=THR,
                 mn=MIN, step=STEP, mx=MAX, set_scene=True, options=None):
    """`k`: the scene's key in adaptive_sim; `options`: ready-made rt_options (their accel and reserved
    words; the stream and the sample base are set here)."""
    opt = lib.make_options(accel=accel) if options is None else type(options).from_buffer_copy(options)
    opt.rng_mode, opt.sample_base = HASH, base
    if set_scene:
        renderer.set_scene(sim.scene(oracle, k))
    iw, ih = image if image else (W, H)
    rci = lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(mx, iw, ih).tobytes())
    acc = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda")
    out = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    info = renderer.render_adaptive(rci, acc, out, sample_count=cnt, rows=rows_t,
                                    options=opt, adaptive=lib.make_adaptive(thr, mn, step))
    torch.cuda.synchronize()
    return acc.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), info


def gpu_plain(lib, renderer, torch, oracle, W, H, spp, base=0):
    rci = lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    renderer.render_device(rci, acc, out, options=lib.make_options(rng_mode=HASH, sample_base=base))
    torch.cuda.synchronize()
    return acc.cpu().numpy(), out.cpu().numpy()


def assert_frame(got, counts, info_sim, ref):
    acc, out, cnt, info = got
    np.testing.assert_array_equal(cnt, counts)
    bad = np.argwhere(acc != ref[0])
    assert bad.size == 0, f"{len(bad)} accumulator floats differ, first at {bad[:4].tolist()}"
    np.testing.assert_array_equal(out, ref[1])
    assert (info.passes, info.tiles, info.tiles_capped, info.samples, info.reserved) == \
        (info_sim["passes"], info_sim["tiles"], info_sim["tiles_capped"], info_sim["samples"], 0)


def parity(lib, renderer, torch, oracle, W, H, vacuous_check=True, **kw):
    """One adaptive frame against the simulation and the oracle."""
    sk = {k: kw[k] for k in ("k", "rows", "base", "image") if k in kw}   # (`options` in kw goes to gpu_adaptive)
    mn, step, mx = kw.get("mn", MIN), kw.get("step", STEP), kw.get("mx", MAX)
    Q = sim.cube(oracle, W, H, mx, **sk)
    counts, info_sim = sim.simulate(Q, mn, step, mx, lib.threshold_q16(kw.get("thr", THR)))
    if vacuous_check:
        sim.assert_not_vacuous(counts, mx)
    ref = sim.expected_frame(oracle, counts, **sk)
    got = gpu_adaptive(lib, renderer, torch, oracle, W, H, **kw)
    assert_frame(got, counts, info_sim, ref)
    return counts, got


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [BRUTE, AUTO])
@pytest.mark.parametrize("shape", [(64, 40), (44, 27)])
def test_simulation_parity(lib, renderer, torch, oracle, shape, accel):
    """The count map equals the simulation, every texel equals oracle.render at its tile's count."""
    counts, _ = parity(lib, renderer, torch, oracle, *shape, accel=accel)
    assert sim.histogram(counts) == ({8: 1, 16: 2, 24: 4, 32: 15, 40: 7, 48: 3, 56: 3, 64: 5} if shape == (64, 40)
                                     else {16: 1, 24: 1, 32: 4, 40: 5, 48: 2, 56: 5, 64: 6})


@pytest.mark.gpu
def test_device_built_scene(lib, renderer, torch, oracle):
    """1 160 spheres: the device build with its L2 grid / treelet walks. Threshold 0.2 chosen on the
    CPU simulation: {8: 1, 24: 1, 32: 5, 40: 2, 48: 4, 56: 6, 64: 5}."""
    parity(lib, renderer, torch, oracle, 44, 27, k=17)
    assert renderer.scene_array(8)["device_built"]


@pytest.mark.gpu
def test_threshold_zero_is_the_uniform_frame(lib, renderer, torch, oracle):
    W, H = 44, 27
    acc, out, cnt, info = gpu_adaptive(lib, renderer, torch, oracle, W, H, thr=0.0)
    pa, po = gpu_plain(lib, renderer, torch, oracle, W, H, MAX)
    assert np.array_equal(acc, pa) and np.array_equal(out, po)
    assert (cnt == MAX).all() and info.passes == 8 and info.tiles_capped == info.tiles == 24
    assert info.samples == MAX * W * H


@pytest.mark.gpu
def test_threshold_sixteen_stops_after_pass_zero(lib, renderer, torch, oracle):
    W, H = 44, 27
    acc, out, cnt, info = gpu_adaptive(lib, renderer, torch, oracle, W, H, thr=16.0)
    pa, po = gpu_plain(lib, renderer, torch, oracle, W, H, MIN)
    assert np.array_equal(acc, pa) and np.array_equal(out, po)
    assert (cnt == MIN).all() and info.passes == 1 and info.tiles_capped == 0
    assert info.samples == MIN * W * H


@pytest.mark.gpu
@pytest.mark.parametrize("base", [0, 1000])
def test_band_with_rows_map(lib, renderer, torch, oracle, base):
    """Non-contiguous rows of a 44x40 image (offset.x = 0), and a sample base."""
    rows = np.array([37, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19, 24, 25, 31, 32, 33, 39], np.int32)
    parity(lib, renderer, torch, oracle, 44, len(rows), rows=rows, base=base, image=(44, 40), vacuous_check=False)


@pytest.mark.gpu
def test_sample_base_on_the_whole_frame(lib, renderer, torch, oracle):
    counts, _ = parity(lib, renderer, torch, oracle, 44, 27, base=1000)
    assert sim.histogram(counts) == {16: 1, 24: 1, 32: 4, 40: 2, 48: 8, 56: 4, 64: 4}


@pytest.mark.gpu
@pytest.mark.parametrize("mn,step,mx", [(8, 8, 60), (8, 16, 64), (8, 16, 60)])
def test_odd_cap_and_step(lib, renderer, torch, oracle, mn, step, mx):
    """max = 60: the last pass is 4 samples (step 8) or 4 after 8 + 3 x 16; step = 16 with min = 8."""
    counts, _ = parity(lib, renderer, torch, oracle, 44, 27, mn=mn, step=step, mx=mx)
    assert counts.max() == mx


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 7])
def test_order_and_chunk_independence(lib, renderer, torch, oracle, chunks):
    renderer.tune(sample_chunks=chunks)
    try:
        parity(lib, renderer, torch, oracle, 64, 40)
    finally:
        renderer.tune(sample_chunks=None)


@pytest.mark.gpu
def test_hygiene_between_adaptive_and_plain_calls(lib, renderer, torch, oracle):
    """The half-buffers are zero and no tile state is stale after an adaptive call, and a plain
    launch leaves nothing an adaptive call could pick up."""
    def plain(W, H, spp):
        pa, po = gpu_plain(lib, renderer, torch, oracle, W, H, spp)
        ra, ro, _ = oracle.render(sim.scene(oracle), oracle.render_call_info(spp, W, H), W, H,
                                  opts=oracle.options(rng_mode=HASH))
        assert np.array_equal(pa, ra) and np.array_equal(po, ro)
    parity(lib, renderer, torch, oracle, 64, 40)
    plain(64, 40, 6)
    parity(lib, renderer, torch, oracle, 44, 27, set_scene=False)    # smaller band, same renderer
    parity(lib, renderer, torch, oracle, 64, 40, set_scene=False)
    plain(44, 27, 5)
    parity(lib, renderer, torch, oracle, 44, 27, set_scene=False)
    plain(64, 40, 6)


@pytest.mark.gpu
def test_refusals(lib, renderer, torch, oracle):
    from rtvk import RtError, abi
    renderer.set_scene(sim.scene(oracle))
    W, H = 16, 8
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    def refused(field, spp=MAX, ad=None, **opt):
        rci = lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())
        o = dict(rng_mode=HASH)
        o.update(opt)
        with pytest.raises(RtError) as e:
            renderer.render_adaptive(rci, acc, out, options=lib.make_options(**o),
                                     adaptive=ad or lib.make_adaptive(THR, MIN, STEP))
        assert e.value.code == -1 and field in str(e.value), str(e.value)   # RT_ERR_INVALID_ARGUMENT

    refused("rng_mode", rng_mode=abi.RT_RNG_PIXEL_STREAM)
    refused("rng_mode", rng_mode=abi.RT_RNG_SAMPLE_COUNTER)
    refused("accumulate", accumulate=True)
    refused("min_spp", ad=lib.make_adaptive(THR, 7, 8))
    refused("min_spp", ad=lib.make_adaptive(THR, 0, 8))
    refused("step_spp", ad=lib.make_adaptive(THR, 8, 3))
    refused("step_spp", ad=lib.make_adaptive(THR, 8, 0))
    refused("max_spp", spp=63)
    refused("min_spp", spp=4)                         # min > max
    refused("threshold", ad=lib.make_adaptive(float("nan"), 8, 8))
    refused("threshold", ad=lib.make_adaptive(float("inf"), 8, 8))
    refused("threshold", ad=lib.make_adaptive(-0.5, 8, 8))
    refused("threshold", ad=lib.make_adaptive(16.5, 8, 8))
    refused("sample_base", sample_base=0xffffffff)
    refused("2^19", spp=(1 << 19) + 2)
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0.0    # nothing rendered
    parity(lib, renderer, torch, oracle, 44, 27, set_scene=False)   # and nothing left behind
