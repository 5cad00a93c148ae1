"""The variance-guided denoise on the GPU (rt_denoise_variance_device) against the
numpy restatement (tests/denoise_var_sim.py), bit for bit: out_mean against denoise_var_sim.denoise
as uint32 views, out_rgba8 against oracle.resolve(mean, 1). The kernels' thread block is 32 x 8
texels and the largest halo staged in LDS is 8 texels (step 4), so the large shape, 83 x 45, is
wider and taller than a block and its halo (48 x 24) and ragged on both sides. Every case runs the
default form (LDS for steps 1, 2 and 4, global memory beyond) and the forced global-memory form,
which must give the same bits."""
import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv
from test_gpu_parity import HASH

pytestmark = pytest.mark.gpu

BLOCK = (32, 8)
LDS_HALO = 8
BIG = (83, 45)
assert BIG[0] > BLOCK[0] + 2 * LDS_HALO and BIG[1] > BLOCK[1] + 2 * LDS_HALO
SHAPES = ((1, 1), (3, 2), (37, 19), BIG)
PASSES = ((0, 1), (2, 3), (3, 6))                  # (prefilter, iterations)
STOPS = ((4.0, 16.0, 0.25), (4.0, 16.0, 0.0), (0.0, 0.0, 0.0))


def sim_params(pre, it, k):
    return (it, pre) + tuple(k)


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


def gpu_denoise(rtvk, torch, r, A, B, feat0, feat1, F, params=None, half_spp=None, half_count=None, stream=None,
                sync=True):
    H, W = A.shape[:2]
    dev = [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (A, B, feat0, feat1)]
    cnt = None if half_count is None else torch.tensor(np.asarray(half_count).astype(np.int32), device="cuda")
    mean = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    p = None if params is None else rtvk.make_denoise_variance(*params)
    torch.cuda.synchronize()      # the buffers' fills ran on torch's stream, the denoise may run on another
    r.denoise_variance(dev[0], dev[1], dev[2], dev[3], F, out, half_spp=half_spp, half_count=cnt, out_mean=mean,
                       params=p, stream=stream)
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
    """Random finite half accumulators and features (no scene smoothness to lean on): (prefilter,
    iterations) (0, 1), (2, 3) and (3, 6); the defaults, k_color = 0 and every k = 0; the default
    form and every launch forced to global memory; a uniform half_spp and a per-texel half_count
    table holding zeros."""
    W, H = shape
    F = 5
    A, B, feat0, feat1 = dv.random_halves(100 + W, H, W, F)
    counts = np.random.default_rng(W).integers(0, 4, (H, W)).astype(np.uint32) * 3
    if counts.size > 1:
        counts.flat[::5] = 0
    try:
        for pre, it in PASSES:
            for k in STOPS:
                params = sim_params(pre, it, k)
                want = dv.denoise(A, B, feat0, feat1, F, half_spp=7, params=params)
                want_c = dv.denoise(A, B, feat0, feat1, F, half_count=counts, params=params)
                assert np.isfinite(want).all() and np.isfinite(want_c).all()
                for lds in (4, 0):
                    renderer.denoise_lds_steps(lds)
                    mean, out = gpu_denoise(rtvk, torch, renderer, A, B, feat0, feat1, F, params, half_spp=7)
                    assert_same(oracle, mean, out, want, (shape, params, lds, "half_spp"))
                    mean, out = gpu_denoise(rtvk, torch, renderer, A, B, feat0, feat1, F, params, half_count=counts)
                    assert_same(oracle, mean, out, want_c, (shape, params, lds, "half_count"))
    finally:
        renderer.denoise_lds_steps(4)


def test_lds_switch_at_every_step(rtvk, torch, renderer, oracle):
    """The switch between the LDS and the global-memory form at steps 1, 2 and 4 changes no bit, in
    the prefilter passes (steps 1, 2, 4) and the iterations (steps 1, 2, 4, 8) alike."""
    W, H = BIG
    A, B, feat0, feat1 = dv.random_halves(7, H, W, 16)
    params = (4, 3, 4.0, 16.0, 0.25)
    want = dv.denoise(A, B, feat0, feat1, 16, half_spp=4, params=params)
    assert np.isfinite(want).all()
    try:
        for lds in (0, 1, 2, 4):
            renderer.denoise_lds_steps(lds)
            mean, out = gpu_denoise(rtvk, torch, renderer, A, B, feat0, feat1, 16, params, half_spp=4)
            assert_same(oracle, mean, out, want, lds)
    finally:
        renderer.denoise_lds_steps(4)


@pytest.mark.parametrize("shape", [(40, 24), (37, 19)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_real_frame_halves_and_features(rtvk, torch, renderer, oracle, shape):
    """An 8-spp frame of the counter-based stream as two halves (render_halves), 16-sample features
    and the filter, all queued on one stream. Each half is the oracle's frame of 4 samples at
    sample_base 0 and 4, the features are the restatement's, the mean is the restatement's of
    them; params=None is the documented default."""
    W, H = shape
    spp, F = 8, 16
    rci = rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())
    s = torch.cuda.Stream()
    z = lambda dt, c=4: torch.zeros((H, W, c), dtype=dt, device="cuda")
    acc_a, acc_b, f0, f1, mean = (z(torch.float32) for _ in range(5))
    out, scratch = z(torch.uint8), z(torch.uint8)
    torch.cuda.synchronize()
    renderer.render_halves(rci, acc_a, acc_b, scratch, stream=s)
    renderer.render_features(rci, f0, f1, samples=F, stream=s)
    renderer.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean, stream=s)
    s.synchronize()
    a, b, g0, g1 = (t.cpu().numpy() for t in (acc_a, acc_b, f0, f1))
    sc = oracle.generate_scene()
    half_rci = oracle.render_call_info(spp // 2, W, H)
    for got, base in ((a, 0), (b, spp // 2)):
        ref, _, _ = oracle.render(sc, half_rci, W, H, opts=oracle.options(rng_mode=HASH, sample_base=base))
        np.testing.assert_array_equal(got, ref, err_msg=f"half at sample_base {base}")
    r0, r1 = ds.features(oracle, sc, oracle.render_call_info(spp, W, H), W, H, F)
    np.testing.assert_array_equal(g0.view(np.uint32), r0.view(np.uint32))
    np.testing.assert_array_equal(g1.view(np.uint32), r1.view(np.uint32))
    want = dv.denoise(a, b, g0, g1, F, half_spp=spp // 2, params=dv.DEFAULTS)
    assert np.isfinite(want).all()
    assert_same(oracle, mean.cpu().numpy(), out.cpu().numpy(), want, (shape, "params=None"))
    renderer.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean,
                              params=rtvk.make_denoise_variance(), stream=s)
    s.synchronize()
    assert_same(oracle, mean.cpu().numpy(), out.cpu().numpy(), want, (shape, "make_denoise_variance()"))
    with pytest.raises(ValueError):       # an odd sample count has no halves
        odd = rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(7, W, H).tobytes())
        renderer.render_halves(odd, acc_a, acc_b, scratch, stream=s)
    with pytest.raises(ValueError):       # the hash stream only
        renderer.render_halves(rci, acc_a, acc_b, scratch, options=rtvk.make_options(), stream=s)


def test_back_to_back_calls_of_different_shapes_and_no_host_waits(rtvk, torch, oracle):
    """Two denoises queued back to back on one stream, the second on a larger band (the context's
    band planes grow under the first): both results are right. With the planes standing, further
    calls of either shape queue without a host wait."""
    F = 4
    small = dv.random_halves(31, 19, 37, F)
    large = dv.random_halves(32, BIG[1], BIG[0], F)
    with rtvk.Renderer(0) as r:
        r.set_scene(oracle.generate_scene())
        s = torch.cuda.Stream()
        m0, o0, keep0, _ = gpu_denoise(rtvk, torch, r, *small, F, dv.DEFAULTS, half_spp=4, stream=s, sync=False)
        m1, o1, keep1, _ = gpu_denoise(rtvk, torch, r, *large, F, dv.DEFAULTS, half_spp=4, stream=s, sync=False)
        s.synchronize()
        assert_same(oracle, m0.cpu().numpy(), o0.cpu().numpy(), dv.denoise(*small, F, half_spp=4), "small")
        assert_same(oracle, m1.cpu().numpy(), o1.cpu().numpy(), dv.denoise(*large, F, half_spp=4), "large")
        waits = r.host_waits()
        for _ in range(2):
            r.denoise_variance(*keep1, F, o1, half_spp=4, out_mean=m1, stream=s)
            r.denoise_variance(*keep0, F, o0, half_spp=4, out_mean=m0, stream=s)
        s.synchronize()
        assert r.host_waits() == waits
        assert_same(oracle, m0.cpu().numpy(), o0.cpu().numpy(), dv.denoise(*small, F, half_spp=4), "small again")
        assert_same(oracle, m1.cpu().numpy(), o1.cpu().numpy(), dv.denoise(*large, F, half_spp=4), "large again")


def test_refusals(rtvk, torch, renderer):
    z = torch.zeros((8, 16, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((8, 16, 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((8, 16), dtype=torch.int32, device="cuda")
    mk = rtvk.make_denoise_variance
    for params, F in ((mk(iterations=0), 4), (mk(iterations=7), 4), (mk(prefilter=4), 4), (mk(k_depth=-1.0), 4),
                      (mk(k_color=float("nan")), 4), (None, 0), (None, 257)):
        with pytest.raises(rtvk.RtError) as e:
            renderer.denoise_variance(z, z, z, z, F, out, half_spp=1, params=params)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        renderer.denoise_variance(z, z, z, z, 4, out)
    with pytest.raises(ValueError):
        renderer.denoise_variance(z, z, z, z, 4, out, half_spp=1, half_count=cnt)


def test_plain_denoise_is_untouched_by_a_variance_denoise(rtvk, torch, oracle):
    """rt_denoise_device before and after a variance denoise on one context, in both kernel forms:
    the same bits, those of its own restatement. The shared band planes (whose w slot the variance
    filter fills) and the LDS switch leak nothing."""
    W, H = BIG
    F = 5
    A, B, feat0, feat1 = dv.random_halves(11, H, W, F)
    want_plain = ds.denoise(A, feat0, feat1, F, spp=7)
    want_var = dv.denoise(A, B, feat0, feat1, F, half_spp=7, params=(4, 3, 4.0, 16.0, 0.25))
    assert np.isfinite(want_plain).all() and np.isfinite(want_var).all()

    def plain(r):
        dev = [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (A, feat0, feat1)]
        mean = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.denoise(dev[0], dev[1], dev[2], F, out, spp=7, out_mean=mean)
        torch.cuda.synchronize()
        return mean.cpu().numpy(), out.cpu().numpy()

    with rtvk.Renderer(0) as r:
        r.set_scene(oracle.generate_scene())
        for lds in (4, 0):
            r.denoise_lds_steps(lds)
            before = plain(r)
            assert_same(oracle, *before, want_plain, ("plain before", lds))
            mean, out = gpu_denoise(rtvk, torch, r, A, B, feat0, feat1, F, (4, 3, 4.0, 16.0, 0.25), half_spp=7)
            assert_same(oracle, mean, out, want_var, ("variance", lds))
            after = plain(r)
            np.testing.assert_array_equal(after[0].view(np.uint32), before[0].view(np.uint32))
            np.testing.assert_array_equal(after[1], before[1])
