"""The reprojected temporal call on the GPU (rt_temporal_reproject_device) against
the numpy restatement (tests/temporal_reproject_sim.py), bit for bit on every output plane; the state
is checked as the next frame sees it, so every sequence runs three frames (the plane sets flip twice).
The motion planes take every branch of the kernel (test_temporal_reproject_sim.branch_motion: the
snap and its edge, four taps, taps that leave the band on each side, ok = 0, NaN and infinity); the
kernel's thread block is 32 x 8 texels, so 33 x 9 is one texel past a block in each direction and
37 x 21 is ragged in both. The real chain runs the whole frame loop of a moving camera at 48 x 32."""
import ctypes

import numpy as np
import pytest

import denoise_var_sim as dv
import motion_sim as ms
import temporal_reproject_sim as tr
import temporal_sim as ts
from test_gpu_parity import HASH
from test_motion_host import moved_camera
from test_temporal_reproject_sim import branch_motion, frames

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = ((33, 9), (37, 21))


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


def gpu_call(rtvk, torch, r, T, A, feat0, feat1, F, motion=None, B=None, spp=None, counts=None, params=None, rgba=True,
             length=True):
    """One call on the GPU (reprojected when a motion plane is given, else in place) with fresh device
    copies of the inputs and outputs prefilled with values no result holds. Returns numpy (out_a, out_b
    or None, rgba8 or None, history_len or None)."""
    H, W = A.shape[:2]
    up = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")
    dA, dB, d0, d1, dM = up(A), up(B), up(feat0), up(feat1), up(motion)
    cnt = None if counts is None else torch.tensor(np.asarray(counts).astype(np.int32), device="cuda")
    out_a = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out_b = None if B is None else torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda") if rgba else None
    hlen = torch.full((H, W), -1, dtype=torch.int32, device="cuda") if length else None
    p = None if params is None else rtvk.make_temporal(*params)
    torch.cuda.synchronize()
    kw = dict(accum_b=dB, out_b=out_b, out_rgba8=out8, history_len=hlen, spp=spp, sample_count=cnt, params=p)
    if motion is None:
        r.temporal_accumulate(T, dA, d0, d1, F, out_a, **kw)
    else:
        r.temporal_reproject(T, dA, d0, d1, F, dM, out_a, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (out_a, out_b, out8, hlen))


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
    """Three frames (A, B, feat0, feat1, motion, counts): smooth guides that change on some texels at
    frames 1 and 2, a branch-covering motion plane per frame, counts with zeros from frame 1 on (a texel
    that keeps its own history, one whose history the guide refuses, one with ok = 0)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (A, B, feat0, feat1) in enumerate(frames(seed, H, W, F)):
        feat1 = feat1.copy()
        if k >= 1:
            feat1[::2, ::3, :3] = -feat1[::2, ::3, :3]
        if k == 2:
            feat1[1::2, 1::3, :3] = -feat1[1::2, 1::3, :3]
        motion = branch_motion(H, W, seed + 40 + k)
        motion[5, 5] = [5.5, 5.5, 0.0, 1.0]
        counts = None
        if with_counts:
            counts = rng.integers(1, 4, (H, W)).astype(np.uint32)
            if k:
                counts[0, 0] = counts[5, 5] = counts[1, 1] = 0
        out.append((A, B, feat0, feat1, motion, counts))
    return out


@pytest.mark.parametrize("with_counts", [False, True], ids=["spp", "counts"])
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_three_frame_sequences(rtvk, torch, renderer, oracle, shape, two, with_counts):
    """Frame 0 goes without out_rgba8, frame 1 without history_len, frame 2 with both. Two
    accumulators run with max_history 3, one with the default parameters (params NULL)."""
    W, H = shape
    F = 5
    params = (3, 4.0, 16.0) if two else None
    st = tr.State(H, W)
    lens = []
    with renderer.temporal(W, H) as T:
        for k, (A, B, feat0, feat1, motion, counts) in enumerate(sequence(60 + W + (7 if two else 0), H, W, F, with_counts)):
            kw = dict(spp=None if with_counts else 3, sample_count=counts, params=params or ts.DEFAULTS)
            want = tr.reproject(st, A, feat0, feat1, F, motion, accum_b=B if two else None, **kw)
            assert np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
            got = gpu_call(rtvk, torch, renderer, T, A, feat0, feat1, F, motion=motion, B=B if two else None,
                           spp=None if with_counts else 3, counts=counts, params=params, rgba=k != 0, length=k != 1)
            check_frame(oracle, got, want, (shape, two, with_counts, k))
            lens.append((want[3], st.ha[..., 3].copy()))
    n2, nf = lens[2]
    assert (n2 == 1).any() and (n2 == 3).any() and (nf != np.floor(nf)).any()      # restarts, the cap, blended lengths
    if with_counts:
        assert n2[5, 5] == lens[1][0][5, 5] > 0 and n2[1, 1] == 0


def test_mixed_calls_and_reset(rtvk, torch, renderer, oracle):
    """reproject, accumulate (in place on the set the first call made current), reproject, reset,
    reproject: each against the restatement on one state."""
    W, H, F = 37, 21, 5
    st = tr.State(H, W)
    seq = sequence(17, H, W, F, False)
    with renderer.temporal(W, H) as T:
        for k, (A, B, feat0, feat1, motion, _) in enumerate(seq + seq[:1]):
            if k == 3:
                T.reset()
                st.reset()
            if k == 1:
                want = ts.accumulate(st, A, feat0, feat1, F, accum_b=B, spp=2)
                got = gpu_call(rtvk, torch, renderer, T, A, feat0, feat1, F, B=B, spp=2)
            else:
                want = tr.reproject(st, A, feat0, feat1, F, motion, accum_b=B, spp=2)
                got = gpu_call(rtvk, torch, renderer, T, A, feat0, feat1, F, motion=motion, B=B, spp=2)
            check_frame(oracle, got, want, k)
        assert np.all(got[3] == 1)           # the frame after the reset is a first frame


def test_nothing_moved_is_the_in_place_call(rtvk, torch, renderer, oracle):
    """The real motion plane of a frame against itself: three reprojected frames on one state equal three
    in-place frames on another, bit for bit."""
    W, H, F = 37, 21, 5
    rci = oracle.render_call_info(1, W, H)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    with renderer.motion(W, H) as M:
        renderer.render_motion(M, rtvk.RenderCallInfo.from_buffer_copy(rci.tobytes()), out)
        torch.cuda.synchronize()
    motion = out.cpu().numpy()
    same_bits(motion, ms.motion(oracle, oracle.generate_scene(), rci, W, H), "motion")
    with renderer.temporal(W, H) as Ta, renderer.temporal(W, H) as Tb:
        for k, (A, B, feat0, feat1) in enumerate(frames(4, H, W, F)):
            a = gpu_call(rtvk, torch, renderer, Ta, A, feat0, feat1, F, motion=motion, B=B, spp=2)
            b = gpu_call(rtvk, torch, renderer, Tb, A, feat0, feat1, F, B=B, spp=2)
            for g, w, name in zip(a, b, ("out_a", "out_b", "rgba8", "history_len")):
                np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=f"{name} at frame {k}")
            assert np.all(a[3] == k + 1)


def test_refusals(rtvk, torch, renderer, oracle):
    W, H = 16, 8
    z = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    a, b, f0, f1, mv, oa, ob = (z() for _ in range(7))
    T = renderer.temporal(W, H)
    renderer.temporal_reproject(T, a, f0, f1, 4, mv, oa, spp=1)
    with rtvk.Renderer(0) as other:
        with other.temporal(W, H) as foreign:
            with pytest.raises(rtvk.RtError) as e:
                renderer.temporal_reproject(foreign, a, f0, f1, 4, mv, oa, spp=1)
            assert e.value.code == -1 and "another context" in str(e.value)
    with pytest.raises(ValueError):
        renderer.temporal_reproject(T, a, f0, f1, 4, mv, oa, out_b=ob, spp=1)
    with pytest.raises(ValueError):
        renderer.temporal_reproject(T, a, f0, f1, 4, mv, oa, accum_b=b, spp=1)
    lib = rtvk.load_library()
    P = ctypes.c_void_p
    ptr = lambda t: P(t.data_ptr())
    call = lambda *args: lib.rt_temporal_reproject_device(*args)
    ctx, S = renderer._ctx, T._state
    cases = (((ctx, S, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, None, None, ptr(oa), None, None, None, None), b"motion"),
             ((ctx, S, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, ptr(mv), None, ptr(oa), ptr(ob), None, None, None), b"out_b"),
             ((ctx, S, ptr(a), ptr(b), None, 1, ptr(f0), ptr(f1), 4, ptr(mv), None, ptr(oa), None, None, None, None), b"out_b"),
             ((ctx, S, ptr(a), None, None, 1, None, ptr(f1), 4, ptr(mv), None, ptr(oa), None, None, None, None), b"feat0"),
             ((ctx, None, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, ptr(mv), None, ptr(oa), None, None, None, None), b"temporal"),
             ((None, S, ptr(a), None, None, 1, ptr(f0), ptr(f1), 4, ptr(mv), None, ptr(oa), None, None, None, None), b"ctx"))
    for args, field in cases:
        assert call(*args) == -1 and field in lib.rt_last_error() and b"rt_temporal_reproject_device" in lib.rt_last_error()
    bad = rtvk.make_temporal()
    bad.reserved = 1
    for params, F, field in ((rtvk.make_temporal(max_history=1), 4, "max_history"), (rtvk.make_temporal(k_depth=-1.0), 4, "k_depth"),
                             (rtvk.make_temporal(k_normal=float("nan")), 4, "k_normal"), (bad, 4, "reserved"),
                             (None, 0, "feature_samples"), (None, 257, "feature_samples")):
        with pytest.raises(rtvk.RtError) as e:
            renderer.temporal_reproject(T, a, f0, f1, F, mv, oa, spp=1, params=params)
        assert e.value.code == -1 and field in str(e.value)
    wide = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
    for args in ((wide, f0, f1, 4, mv, oa), (a, f0, f1, 4, wide, oa), (a, f0, f1, 4, mv, wide)):
        with pytest.raises(ValueError):
            renderer.temporal_reproject(T, *args, spp=1)
    with pytest.raises(ValueError):
        renderer.temporal_reproject(T, a, f0, f1, 4, mv, oa)
    torch.cuda.synchronize()
    T.close()
    with pytest.raises(ValueError):
        renderer.temporal_reproject(T, a, f0, f1, 4, mv, oa, spp=1)


# ---- a real chain ---------------------------------------------------------------------------------

CHAIN = dict(W=48, H=32, spp=2, F=4, N=4, s=0.2, dt=0.2)


def gpu_chain(rtvk, torch, oracle, frames_n=3, dt=None):
    """Frame k of the canonical scene at time k dt from frame k of the camera path: two halves of 1
    sample at sample_base 2 k and 2 k + 1, the features at sample_base 0, the motion plane, keep_current,
    the reprojected call and the variance filter, all queued on one stream. Returns per frame the GPU's
    own (A, B, feat0, feat1, motion) and (out_a, out_b, mean, rgba8, history_len) as numpy."""
    W, H, spp, F, N, s = (CHAIN[k] for k in ("W", "H", "spp", "F", "N", "s"))
    dt = CHAIN["dt"] if dt is None else dt
    z = lambda dtype, c=4: torch.zeros((H, W, c), dtype=dtype, device="cuda")
    acc_a, acc_b, f0, f1, mv, out_a, out_b, mean = (z(torch.float32) for _ in range(8))
    out, scratch = z(torch.uint8), z(torch.uint8)
    hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    params = rtvk.make_temporal(max_history=N)
    st = torch.cuda.Stream()
    ins, outs = [], []
    torch.cuda.synchronize()
    with rtvk.Renderer(0) as r, torch.cuda.stream(st):
        T, M = r.temporal(W, H), r.motion(W, H)
        for k in range(frames_n):
            rci_np = moved_camera(oracle, spp, W, H, s, k)
            rci = rtvk.RenderCallInfo.from_buffer_copy(rci_np.tobytes())
            r.set_scene(oracle.generate_scene(float(f32(k * dt))), stream=st)
            r.render_halves(rci, acc_a, acc_b, scratch, options=rtvk.make_options(rng_mode=HASH, sample_base=spp * k), stream=st)
            r.render_features(rci, f0, f1, samples=F, stream=st)
            r.render_motion(M, rci, mv, stream=st)
            M.keep_current(rci, stream=st)
            r.temporal_reproject(T, acc_a, f0, f1, F, mv, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen,
                                 spp=spp // 2, params=params, stream=st)
            r.denoise_variance(out_a, out_b, f0, f1, F, out, half_spp=1, out_mean=mean, stream=st)
            st.synchronize()
            ins.append(tuple(t.cpu().numpy() for t in (acc_a, acc_b, f0, f1, mv)) + (rci_np,))
            outs.append(tuple(t.cpu().numpy() for t in (out_a, out_b, mean, out, hlen)))
        T.close()
        M.close()
    return ins, outs


def test_real_chain(rtvk, torch, oracle):
    """Three frames of the moving scene under the moving camera: every frame's motion plane equals the
    restatement's, and the reprojected call and the filter equal the restatement chain on the GPU's own
    buffers, plane by plane and byte by byte; at frame 2 most histories hold three frames."""
    W, H, spp, F, N, s, dt = (CHAIN[k] for k in ("W", "H", "spp", "F", "N", "s", "dt"))
    ins, outs = gpu_chain(rtvk, torch, oracle)
    st = tr.State(H, W)
    prev = None
    for k, ((A, B, feat0, feat1, mv, rci_np), (out_a, out_b, mean, out8, hlen)) in enumerate(zip(ins, outs)):
        sc = oracle.generate_scene(float(f32(k * dt)))
        want_mv = ms.motion(oracle, sc, rci_np, W, H, *(prev or (None, None)))
        same_bits(mv, want_mv, (k, "motion"))
        prev = (sc, rci_np)
        w_a, w_b, _, w_n = tr.reproject(st, A, feat0, feat1, F, mv, accum_b=B, spp=spp // 2, params=(N, 4.0, 16.0))
        w_mean = dv.denoise(w_a, w_b, feat0, feat1, F, half_spp=1)
        assert np.isfinite(w_mean).all()
        same_bits(out_a, w_a, (k, "out_a"))
        same_bits(out_b, w_b, (k, "out_b"))
        same_bits(mean, w_mean, (k, "mean"))
        np.testing.assert_array_equal(out8, oracle.resolve(w_mean, 1))
        np.testing.assert_array_equal(hlen.astype(np.uint32), w_n)
    n = outs[2][4]
    assert np.all(outs[0][4] == 1) and (n == 3).mean() > 0.5 and (n == 1).any()
    # the camera moved: the planes were fetched from other texels
    assert np.abs(ins[2][4][..., 0] - (np.arange(W) + 0.5)[None, :]).max() > 0.5
