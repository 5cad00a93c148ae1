"""The edge-avoiding denoise on the GPU (rt_denoise_device) against the numpy
restatement (tests/denoise_sim.py), bit for bit: out_mean against denoise_sim.denoise, out_rgba8
against oracle.resolve(mean, 1). The kernels' thread block is 32 x 8 texels and the largest halo
staged in LDS is 8 texels (step 4), so the large shape, 83 x 45, is wider and taller than a block
and its halo (48 x 24) and ragged on both sides; with it every step from 1 to 32 skips taps on all
four borders. Every case runs the default form (LDS for steps 1, 2 and 4, global memory beyond) and
the forced forms, which must give the same bits."""
import numpy as np
import pytest

import denoise_sim as ds
from test_gpu_parity import HASH

pytestmark = pytest.mark.gpu

BLOCK = (32, 8)
LDS_HALO = 8
BIG = (83, 45)
assert BIG[0] > BLOCK[0] + 2 * LDS_HALO and BIG[1] > BLOCK[1] + 2 * LDS_HALO
SHAPES = ((1, 1), (3, 2), (40, 24), (37, 19), BIG)
PARAMS = ((4.0, 16.0, 1.0), (4.0, 16.0, 0.0), (0.0, 0.0, 0.0))
ITERATIONS = (1, 3, 6)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rtvk(torch):
    import rtvk as m
    return m


@pytest.fixture(scope="module")
def renderer(rtvk, oracle):
    r = rtvk.Renderer(0)
    r.set_scene(oracle.generate_scene())
    yield r
    r.close()


def gpu_denoise(rtvk, torch, r, accum, feat0, feat1, F, params=None, spp=None, sample_count=None, stream=None,
                sync=True):
    H, W = accum.shape[:2]
    dev = [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (accum, feat0, feat1)]
    cnt = None if sample_count is None else torch.tensor(np.asarray(sample_count).astype(np.int32), device="cuda")
    mean = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    p = None if params is None else rtvk.make_denoise(*params)
    torch.cuda.synchronize()      # the buffers' fills ran on torch's stream, the denoise may run on another
    r.denoise(dev[0], dev[1], dev[2], F, out, spp=spp, sample_count=cnt, out_mean=mean, params=p, stream=stream)
    if not sync:
        return mean, out, dev, cnt
    torch.cuda.synchronize()
    return mean.cpu().numpy(), out.cpu().numpy()


def assert_same(oracle, mean, out, want, what):
    g, w = np.ascontiguousarray(mean).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), mean[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
    np.testing.assert_array_equal(out, oracle.resolve(want, 1), err_msg=str(what))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_inputs_every_form(rtvk, torch, renderer, oracle, shape):
    """Random finite accumulators and features (no scene smoothness to lean on): iterations 1, 3 and
    6, the defaults, k_color = 0 and every k = 0, in the default form and with every iteration forced
    to global memory; a uniform spp and a per-texel count table holding zeros."""
    W, H = shape
    F = 5
    accum, feat0, feat1 = ds.random_inputs(100 + W, H, W, F)
    counts = np.random.default_rng(W).integers(0, 4, (H, W)).astype(np.uint32) * 3
    if counts.size > 1:
        counts.flat[::5] = 0
    try:
        for it in ITERATIONS:
            for k in PARAMS:
                params = (it,) + k
                want = ds.denoise(accum, feat0, feat1, F, spp=7, params=params)
                want_c = ds.denoise(accum, feat0, feat1, F, sample_count=counts, params=params)
                assert np.isfinite(want).all() and np.isfinite(want_c).all()
                for lds in (4, 0):
                    renderer.denoise_lds_steps(lds)
                    mean, out = gpu_denoise(rtvk, torch, renderer, accum, feat0, feat1, F, params, spp=7)
                    assert_same(oracle, mean, out, want, (shape, params, lds, "spp"))
                    mean, out = gpu_denoise(rtvk, torch, renderer, accum, feat0, feat1, F, params, sample_count=counts)
                    assert_same(oracle, mean, out, want_c, (shape, params, lds, "counts"))
    finally:
        renderer.denoise_lds_steps(4)


def test_lds_switch_at_every_step(rtvk, torch, renderer, oracle):
    """The switch between the LDS and the global-memory form at steps 1, 2 and 4 changes no bit."""
    W, H = BIG
    accum, feat0, feat1 = ds.random_inputs(7, H, W, 16)
    want = ds.denoise(accum, feat0, feat1, 16, spp=8, params=(4, 4.0, 16.0, 1.0))
    try:
        for lds in (0, 1, 2, 4):
            renderer.denoise_lds_steps(lds)
            mean, out = gpu_denoise(rtvk, torch, renderer, accum, feat0, feat1, 16, (4, 4.0, 16.0, 1.0), spp=8)
            assert_same(oracle, mean, out, want, lds)
        with pytest.raises(rtvk.RtError):
            renderer.denoise_lds_steps(3)
    finally:
        renderer.denoise_lds_steps(4)


def rendered(rtvk, torch, r, oracle, W, H, spp, F):
    rci = rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    f0 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    f1 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    return rci, acc, out, f0, f1


@pytest.mark.parametrize("shape", [(40, 24), (37, 19)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_real_frame_and_features(rtvk, torch, renderer, oracle, shape):
    """An 8-spp frame of the counter-based stream with 16-sample features, as a frame loop runs
    them: frame, features and denoise queued on one stream. The frame and the features are the
    oracle's and the restatement's, the denoised mean is the restatement's of them."""
    W, H = shape
    spp, F = 8, 16
    rci, acc, out, f0, f1 = rendered(rtvk, torch, renderer, oracle, W, H, spp, F)
    mean = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.render_device(rci, acc, out, options=rtvk.make_options(rng_mode=HASH))
    renderer.render_features(rci, f0, f1, samples=F)
    for it in ITERATIONS:
        renderer.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean, params=rtvk.make_denoise(iterations=it))
        torch.cuda.synchronize()
        a, g0, g1 = acc.cpu().numpy(), f0.cpu().numpy(), f1.cpu().numpy()
        want = ds.denoise(a, g0, g1, F, spp=spp, params=(it,) + ds.DEFAULTS[1:])
        assert_same(oracle, mean.cpu().numpy(), out.cpu().numpy(), want, (shape, it))
    sc = oracle.generate_scene()
    ref_acc, _, _ = oracle.render(sc, oracle.render_call_info(spp, W, H), W, H, opts=oracle.options(rng_mode=HASH))
    r0, r1 = ds.features(oracle, sc, oracle.render_call_info(spp, W, H), W, H, F)
    np.testing.assert_array_equal(a, ref_acc)
    np.testing.assert_array_equal(g0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(g1.view(np.uint32), r1.view(np.uint32))
    # params = None is the documented default
    renderer.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean)
    torch.cuda.synchronize()
    assert_same(oracle, mean.cpu().numpy(), out.cpu().numpy(), ds.denoise(a, g0, g1, F, spp=spp), (shape, "default"))


def test_adaptive_frame_with_its_sample_counts(rtvk, torch, renderer, oracle):
    W, H, F = 64, 40, 16      # the frame of test_cli_adaptive.py: tiles stop at different counts
    rci, acc, out, f0, f1 = rendered(rtvk, torch, renderer, oracle, W, H, 64, F)
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    mean = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.render_adaptive(rci, acc, out, sample_count=cnt, options=rtvk.make_options(rng_mode=HASH),
                             adaptive=rtvk.make_adaptive(0.2, min_spp=8, step_spp=8))
    renderer.render_features(rci, f0, f1, samples=F)
    renderer.denoise(acc, f0, f1, F, out, sample_count=cnt, out_mean=mean)
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy().astype(np.uint32)
    assert counts.min() >= 8 and len(np.unique(counts)) > 1      # the frame is adaptive
    want = ds.denoise(acc.cpu().numpy(), f0.cpu().numpy(), f1.cpu().numpy(), F, sample_count=counts)
    assert_same(oracle, mean.cpu().numpy(), out.cpu().numpy(), want, "adaptive")


def test_back_to_back_calls_of_different_shapes_and_no_host_waits(rtvk, torch, oracle):
    """Two denoises queued back to back on one stream, the second on a larger band (the context's
    band buffers grow under the first): both results are right. With the buffers standing, features
    plus denoise queue without a host wait."""
    F = 4
    small = ds.random_inputs(31, 19, 37, F)
    large = ds.random_inputs(32, BIG[1], BIG[0], F)
    with rtvk.Renderer(0) as r:
        r.set_scene(oracle.generate_scene())
        s = torch.cuda.Stream()
        m0, o0, keep0, _ = gpu_denoise(rtvk, torch, r, *small, F, (3, 4.0, 16.0, 1.0), spp=8, stream=s, sync=False)
        m1, o1, keep1, _ = gpu_denoise(rtvk, torch, r, *large, F, (3, 4.0, 16.0, 1.0), spp=8, stream=s, sync=False)
        s.synchronize()
        assert_same(oracle, m0.cpu().numpy(), o0.cpu().numpy(), ds.denoise(*small, F, spp=8), "small")
        assert_same(oracle, m1.cpu().numpy(), o1.cpu().numpy(), ds.denoise(*large, F, spp=8), "large")
        waits = r.host_waits()
        W, H = BIG
        rci = rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(8, W, H).tobytes())
        f0 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        f1 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            r.render_features(rci, f0, f1, samples=F, stream=s)
            r.denoise(keep1[0], f0, f1, F, o1, spp=8, out_mean=m1, stream=s)
            r.denoise(keep0[0], keep0[1], keep0[2], F, o0, spp=8, out_mean=m0, stream=s)
        s.synchronize()
        assert r.host_waits() == waits
        assert_same(oracle, m0.cpu().numpy(), o0.cpu().numpy(), ds.denoise(*small, F, spp=8), "small again")


def test_refusals(rtvk, torch, renderer):
    z = torch.zeros((8, 16, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((8, 16, 4), dtype=torch.uint8, device="cuda")
    for params, F in ((rtvk.make_denoise(iterations=0), 4), (rtvk.make_denoise(iterations=7), 4),
                      (rtvk.make_denoise(k_depth=-1.0), 4), (rtvk.make_denoise(k_color=float("nan")), 4),
                      (None, 0), (None, 257)):
        with pytest.raises(rtvk.RtError) as e:
            renderer.denoise(z, z, z, F, out, spp=1, params=params)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        renderer.denoise(z, z, z, 4, out)
