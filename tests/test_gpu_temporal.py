"""The temporal stage on the GPU (rt_temporal_accumulate_device) against the numpy
restatement (tests/temporal_sim.py), bit for bit on every output plane: out_a and out_b as uint32
views, out_rgba8 against oracle.resolve(mean, 1), history_len as integers. The state itself is
checked as the next frame sees it: every sequence runs three frames and compares each. The kernel's
thread block is 32 x 8 texels, so 33 x 9 is one texel past a block in each direction and 37 x 21 is
ragged in both and no multiple of 64 texels."""
import ctypes

import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv
import temporal_sim as ts
from test_gpu_parity import HASH

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = ((1, 1), (33, 9), (37, 21))


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


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])


def gpu_accumulate(rtvk, torch, r, T, A, feat0, feat1, F, B=None, spp=None, counts=None, params=None, rgba=True,
                   length=True, stream=None, sync=True):
    """One call on the GPU with fresh device copies of the inputs and outputs prefilled with values no
    result holds. Returns numpy (out_a, out_b or None, rgba8 or None, history_len or None)."""
    H, W = A.shape[:2]
    up = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")
    dA, dB, d0, d1 = up(A), up(B), up(feat0), up(feat1)
    cnt = None if counts is None else torch.tensor(np.asarray(counts).astype(np.int32), device="cuda")
    out_a = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out_b = None if B is None else torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda") if rgba else None
    hlen = torch.full((H, W), -1, dtype=torch.int32, device="cuda") if length else None
    p = None if params is None else rtvk.make_temporal(*params)
    torch.cuda.synchronize()      # the fills ran on torch's stream, the call may run on another
    r.temporal_accumulate(T, dA, d0, d1, F, out_a, accum_b=dB, out_b=out_b, out_rgba8=out8, history_len=hlen,
                          spp=spp, sample_count=cnt, params=p, stream=stream)
    outs = (out_a, out_b, out8, hlen)
    if not sync:
        return outs, (dA, dB, d0, d1, cnt)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in outs)


def check_frame(oracle, got, want, what):
    out_a, out_b, out8, hlen = got
    w_a, w_b, w_mean, w_n = want
    same_bits(out_a, w_a, (what, "out_a"))
    assert (out_b is None) == (w_b is None)
    if out_b is not None:
        same_bits(out_b, w_b, (what, "out_b"))
    if out8 is not None:
        np.testing.assert_array_equal(out8, oracle.resolve(w_mean, 1), err_msg=str((what, "rgba8")))
    if hlen is not None:
        np.testing.assert_array_equal(hlen.astype(np.uint32), w_n, err_msg=str((what, "history_len")))


def sequence(seed, H, W, F, with_counts):
    """Three frames of random finite inputs. The guides of a frame equal the frame before's except on
    a seeded third of the texels, whose normal sums are negated or whose depth sum is doubled (normal
    components at least 1 / 4 and depths at least 1 after the division by F, so that either change
    stops the history whatever the draw): both outcomes of `valid` in every block. The sample counts
    hold zeros at the corner and mid-band; at frame 2 the mid-band texel keeps its guide (no samples, a
    valid history) and the last texel loses it (no samples, no valid history)."""
    rng = np.random.default_rng(seed)
    frames = []
    _, _, feat1 = ts.random_inputs(seed, H, W, F)
    feat1[..., :3] = np.where(np.abs(feat1[..., :3]) < F / 4, f32(F / 2), feat1[..., :3])
    feat1[..., 3] = np.maximum(feat1[..., 3], f32(F))
    for k in range(3):
        A, feat0, _ = ts.random_inputs(seed + 10 * k + 1, H, W, F)
        B, _, _ = ts.random_inputs(seed + 10 * k + 2, H, W, F)
        if k > 0:
            feat1 = feat1.copy()
            change = rng.integers(0, 3, (H, W)) == 0
            flip = rng.integers(0, 2, (H, W)) == 0
            if k == 2 and H * W > 1:
                change[H // 2, W // 2] = False
                change[H - 1, W - 1] = True
            feat1[..., :3] = np.where((change & flip)[..., None], -feat1[..., :3], feat1[..., :3])
            feat1[..., 3] = np.where(change & ~flip, feat1[..., 3] * f32(2.0), feat1[..., 3])
        counts = None
        if with_counts:
            counts = rng.integers(1, 5, (H, W)).astype(np.uint32)
            counts[0, 0] = 0
            if k != 1:
                counts[H // 2, W // 2] = 0
            if k == 2:
                counts[H - 1, W - 1] = 0
        frames.append((A, B, feat0, feat1, counts))
    return frames


@pytest.mark.parametrize("with_counts", [False, True], ids=["spp", "counts"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_frame_sequences(rtvk, torch, renderer, oracle, shape, two, with_counts):
    """Frame 0 goes without out_rgba8, frame 1 without history_len, frame 2 with both. Two
    accumulators run with max_history 2 (the cap holds at frame 2), one with the default parameters
    (params NULL)."""
    W, H = shape
    F = 5
    params = (2, 4.0, 16.0) if two else None
    st = ts.State(H, W)
    lens = []
    with renderer.temporal(W, H) as T:
        for k, (A, B, feat0, feat1, counts) in enumerate(sequence(50 + W + (7 if two else 0), H, W, F, with_counts)):
            kw = dict(spp=None if with_counts else 3, params=params or ts.DEFAULTS)
            want = ts.accumulate(st, A, feat0, feat1, F, accum_b=B if two else None, sample_count=counts, **kw)
            assert np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
            got = gpu_accumulate(rtvk, torch, renderer, T, A, feat0, feat1, F, B=B if two else None,
                                 spp=None if with_counts else 3, counts=counts, params=params, rgba=k != 0, length=k != 1)
            check_frame(oracle, got, want, (shape, two, with_counts, k))
            lens.append(want[3])
    for n in lens[1:]:      # both outcomes of `valid` in every block that holds a wave of texels
        for by in range(0, H, 8):
            for bx in range(0, W, 32):
                part = n[by:by + 8, bx:bx + 32]
                if part.size >= 64:
                    measured = part[part > 0]
                    assert (measured == 1).any() and (measured > 1).any(), (by, bx)
    if two and H * W > 64:
        assert lens[2].max() == 2
    if with_counts and H * W > 1:
        assert lens[2][H // 2, W // 2] == lens[1][H // 2, W // 2] > 0 and lens[2][H - 1, W - 1] == 0


def test_the_same_frame_four_times(rtvk, torch, renderer):
    """A static scene whose frames repeat their noise: the outputs are the same bits every time, and
    history_len = min(m, N), N = 3."""
    W, H, F = 37, 21, 5
    A, feat0, feat1 = ts.random_inputs(5, H, W, F)
    B, _, _ = ts.random_inputs(6, H, W, F)
    first = None
    with renderer.temporal(W, H) as T:
        for m in range(1, 5):
            got = gpu_accumulate(rtvk, torch, renderer, T, A, feat0, feat1, F, B=B, spp=2, params=(3, 4.0, 16.0))
            first = first or got
            for g, w, name in zip(got[:3], first[:3], ("out_a", "out_b", "rgba8")):
                np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{name} at call {m}")
            assert np.all(got[3] == min(m, 3)), m
    assert np.all(first[0] != -3.0) and np.all(first[2][..., 3] == 255)


def test_reset(rtvk, torch, renderer, oracle):
    """reset between frames makes the next frame a frame 0; a reset queued on the same stream behind a
    call leaves that call's outputs alone."""
    W, H, F = 37, 21, 5
    (A0, B0, g0, h0, _), (A1, B1, g1, h1, _), _ = sequence(9, H, W, F, False)
    fresh0 = ts.accumulate(ts.State(H, W), A0, g0, h0, F, accum_b=B0, spp=2)
    fresh1 = ts.accumulate(ts.State(H, W), A1, g1, h1, F, accum_b=B1, spp=2)
    s = torch.cuda.Stream()
    with renderer.temporal(W, H) as T:
        outs, keep = gpu_accumulate(rtvk, torch, renderer, T, A0, g0, h0, F, B=B0, spp=2, stream=s, sync=False)
        T.reset(stream=s)
        s.synchronize()
        check_frame(oracle, tuple(t.cpu().numpy() for t in outs), fresh0, "the call ahead of a reset")
        got = gpu_accumulate(rtvk, torch, renderer, T, A1, g1, h1, F, B=B1, spp=2, stream=s)
        check_frame(oracle, got, fresh1, "the frame after a reset")
        assert np.all(got[3] == 1)
        # without the reset the same frame integrates
        got = gpu_accumulate(rtvk, torch, renderer, T, A0, g0, h0, F, B=B0, spp=2, stream=s)
        assert (got[3] == 2).any()
    del keep


def test_refusals(rtvk, torch, renderer, oracle):
    W, H = 16, 8
    z = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    a, b, f0, f1, oa, ob = (z() for _ in range(6))
    T = renderer.temporal(W, H)
    renderer.temporal_accumulate(T, a, f0, f1, 4, oa, spp=1)
    # a state of another Renderer
    with rtvk.Renderer(0) as other:
        with other.temporal(W, H) as foreign:
            with pytest.raises(rtvk.RtError) as e:
                renderer.temporal_accumulate(foreign, a, f0, f1, 4, oa, spp=1)
            assert e.value.code == -1 and "another context" in str(e.value)
    # out_b without accum_b and the reverse: the wrapper, and the library itself
    with pytest.raises(ValueError):
        renderer.temporal_accumulate(T, a, f0, f1, 4, oa, out_b=ob, spp=1)
    with pytest.raises(ValueError):
        renderer.temporal_accumulate(T, a, f0, f1, 4, oa, accum_b=b, spp=1)
    lib = rtvk.load_library()
    P = ctypes.c_void_p
    ptr = lambda t: P(t.data_ptr())
    rc = lib.rt_temporal_accumulate_device(renderer._ctx, T._state, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, None, ptr(oa),
                                           ptr(ob), None, None, None)
    assert rc == -1 and b"out_b" in lib.rt_last_error()
    rc = lib.rt_temporal_accumulate_device(renderer._ctx, T._state, ptr(a), ptr(b), None, 1, ptr(f0), ptr(f1), 4, None,
                                           ptr(oa), None, None, None, None)
    assert rc == -1 and b"out_b" in lib.rt_last_error()
    rc = lib.rt_temporal_accumulate_device(renderer._ctx, T._state, ptr(a), None, None, 1, None, ptr(f1), 4, None, ptr(oa),
                                           None, None, None, None)
    assert rc == -1 and b"feat0" in lib.rt_last_error()
    rc = lib.rt_temporal_accumulate_device(renderer._ctx, None, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, None, ptr(oa),
                                           None, None, None, None)
    assert rc == -1 and b"temporal" in lib.rt_last_error()
    # the parameters, each named
    bad = rtvk.make_temporal()
    bad.reserved = 1
    for params, F, field in ((rtvk.make_temporal(max_history=1), 4, "max_history"), (rtvk.make_temporal(k_depth=-1.0), 4, "k_depth"),
                             (rtvk.make_temporal(k_normal=float("nan")), 4, "k_normal"), (bad, 4, "reserved"),
                             (None, 0, "feature_samples"), (None, 257, "feature_samples")):
        with pytest.raises(rtvk.RtError) as e:
            renderer.temporal_accumulate(T, a, f0, f1, F, oa, spp=1, params=params)
        assert e.value.code == -1 and field in str(e.value)
    # tensors of another band size, neither or both of spp and sample_count
    wide = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
    for args in ((wide, f0, f1, 4, oa), (a, wide, f1, 4, oa), (a, f0, f1, 4, wide)):
        with pytest.raises(ValueError):
            renderer.temporal_accumulate(T, *args, spp=1)
    with pytest.raises(ValueError):
        renderer.temporal_accumulate(T, a, f0, f1, 4, oa, spp=1, history_len=torch.zeros((H, W + 1), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        renderer.temporal_accumulate(T, a, f0, f1, 4, oa)
    with pytest.raises(rtvk.RtError):
        renderer.temporal(0, 8)
    with pytest.raises(rtvk.RtError):
        renderer.temporal(8, 65536)
    # after close
    torch.cuda.synchronize()
    T.close()
    with pytest.raises(ValueError):
        renderer.temporal_accumulate(T, a, f0, f1, 4, oa, spp=1)
    with pytest.raises(ValueError):
        T.reset()
    T.close()      # closing twice is harmless


# ---- a real chain ---------------------------------------------------------------------------------

CHAIN = dict(W=64, H=36, spp=2, F=4, N=4)


def gpu_chain(rtvk, torch, oracle, times, variance):
    """The canonical scene at the times `times`, one frame each: frame k rendered as two halves of 1
    sample at sample_base 2 k and 2 k + 1, its features at sample_base 0, temporal_accumulate and the
    filter, all queued on one stream. variance: the halves go through the temporal call and
    denoise_variance; else their sum goes through it as one accumulator and denoise. Returns
    (frames, mean, rgba8, lens): per frame the GPU's own (A, B, feat0, feat1) as numpy, the last
    frame's filtered mean and bytes, and every frame's history_len."""
    W, H, spp, F, N = (CHAIN[k] for k in ("W", "H", "spp", "F", "N"))
    rci = rtvk.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())
    z = lambda dt, c=4: torch.zeros((H, W, c), dtype=dt, device="cuda")
    acc_a, acc_b, f0, f1, out_a, out_b, mean = (z(torch.float32) for _ in range(7))
    out, scratch = z(torch.uint8), z(torch.uint8)
    hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    params = rtvk.make_temporal(max_history=N)
    s = torch.cuda.Stream()
    frames, lens = [], []
    torch.cuda.synchronize()
    with rtvk.Renderer(0) as r, torch.cuda.stream(s):
        T = r.temporal(W, H)
        for k, t in enumerate(times):
            r.set_scene(oracle.generate_scene(t), stream=s)
            r.render_halves(rci, acc_a, acc_b, scratch, options=rtvk.make_options(rng_mode=HASH, sample_base=spp * k), stream=s)
            r.render_features(rci, f0, f1, samples=F, stream=s)
            if variance:
                r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen,
                                      spp=spp // 2, params=params, stream=s)
                r.denoise_variance(out_a, out_b, f0, f1, F, out, half_spp=1, out_mean=mean, stream=s)
            else:
                acc_a.add_(acc_b)
                r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, history_len=hlen, spp=spp, params=params, stream=s)
                r.denoise(out_a, f0, f1, F, out, spp=1, out_mean=mean, stream=s)
            s.synchronize()
            frames.append(tuple(t_.cpu().numpy() for t_ in (acc_a, acc_b, f0, f1)))
            lens.append(hlen.cpu().numpy().astype(np.uint32))
        T.close()
    return frames, mean.cpu().numpy(), out.cpu().numpy(), lens


def sim_chain(frames, variance):
    """The restatement chain on the buffers gpu_chain returned: (mean, history_len of the last frame)."""
    W, H, spp, F, N = (CHAIN[k] for k in ("W", "H", "spp", "F", "N"))
    st = ts.State(H, W)
    for A, B, feat0, feat1 in frames:
        if variance:
            out_a, out_b, _, n = ts.accumulate(st, A, feat0, feat1, F, accum_b=B, spp=spp // 2, params=(N, 4.0, 16.0))
            mean = dv.denoise(out_a, out_b, feat0, feat1, F, half_spp=1)
        else:       # A already holds the sum of the halves
            out_a, _, _, n = ts.accumulate(st, A, feat0, feat1, F, spp=spp, params=(N, 4.0, 16.0))
            mean = ds.denoise(out_a, feat0, feat1, F, spp=1)
    return mean, n


@pytest.mark.parametrize("variance", [True, False], ids=["variance", "plain"])
def test_real_chain(rtvk, torch, oracle, variance):
    """Three frames of the moving scene (t = 0, 0.2, 0.4): the GPU chain equals the restatement chain
    on the same GPU buffers bit for bit, and at frame 2 some texels hold all three frames and some
    started over."""
    frames, mean, out, lens = gpu_chain(rtvk, torch, oracle, (0.0, 0.2, 0.4), variance)
    want, n = sim_chain(frames, variance)
    assert np.isfinite(want).all()
    same_bits(mean, want, "mean")
    np.testing.assert_array_equal(out, oracle.resolve(want, 1))
    np.testing.assert_array_equal(lens[2], n)
    assert (lens[2] == 1).any() and (lens[2] == 3).any()
    assert np.all(lens[0] == 1)
