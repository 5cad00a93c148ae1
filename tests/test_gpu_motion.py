"""The motion pass on the GPU (rt_render_motion_device) against the numpy
restatement (tests/motion_sim.py), bit for bit on the whole motion plane, for every walk form the
closest-hit probe knows. The trace is the kernels' MODE_PROBE instantiation at the band's own width,
which the probe itself only ever ran at 512 texels without an offset: 40 x 24 is whole tiles in more
than one 64-unit block, 37 x 19 is ragged at the right and bottom edges and sits at offset (9, 5) of a
64 x 36 image. Every case is the canonical scene at t = 0 seen from frame 0 of the s = 0.2 camera path
against a previous frame at t = 0.2 seen from frame 1. The restatement of a shape is computed once."""
import ctypes
import functools

import numpy as np
import pytest

import denoise_sim as ds
import motion_sim as ms
from test_gpu_closest_hit import FORM_NAME, PROBE_FORMS, REGATE
from test_gpu_parity import BRUTE, LBVH, WALK_FORM, tree_builder
from test_motion_host import SNAP, moved_camera

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = {"40x24": (40, 24, 40, 24, (0, 0)), "37x19": (37, 19, 64, 36, (9, 5))}     # band, image, offset


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
    r.set_scene(oracle.generate_scene(0.0))
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def case(oracle, shape):
    """(scene, rci, previous scene, previous rci, the restatement's plane with the previous frame, and
    without one) of a shape."""
    W, H, IW, IH, off = SHAPES[shape]
    sc, prev = oracle.generate_scene(0.0), oracle.generate_scene(0.2)
    rci = moved_camera(oracle, 1, IW, IH, 0.2, 0, offset=off)
    prev_rci = moved_camera(oracle, 1, IW, IH, 0.2, 1, offset=off)
    want = ms.motion(oracle, sc, rci, W, H, prev, prev_rci)
    alone = ms.motion(oracle, sc, rci, W, H)
    for a in (want, alone):
        a.setflags(write=False)
    return sc, rci, prev, prev_rci, want, alone


def options(rtvk, form):
    o = rtvk.make_options(accel=BRUTE if form == BRUTE else LBVH)
    o.reserved[1] = WALK_FORM.get(form, 0)
    if form == REGATE:
        o.reserved[0] |= 2
    return o


def as_rci(rtvk, rci_np):
    return rtvk.RenderCallInfo.from_buffer_copy(np.ascontiguousarray(rci_np).tobytes())


def gpu_motion(rtvk, torch, r, M, rci_np, opt=None):
    out = torch.full((M.height, M.width, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_motion(M, as_rci(rtvk, rci_np), out, options=opt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", PROBE_FORMS, ids=lambda f: FORM_NAME[f])
def test_every_form_matches_the_restatement(rtvk, torch, renderer, oracle, form, shape):
    W, H = SHAPES[shape][:2]
    sc, rci, prev, prev_rci, want, _ = case(oracle, shape)
    with renderer.motion(W, H) as M:
        M.set_previous(prev, as_rci(rtvk, prev_rci))
        got = gpu_motion(rtvk, torch, renderer, M, rci, options(rtvk, form))
    same_bits(got, want, (FORM_NAME[form], shape))
    # the case moves: hits and sky, most texels ok and more than a quarter of a texel from their own centre
    hit = want[..., 2] != 0
    assert 0.5 < hit.mean() and want[..., 3].mean() > 0.9
    assert np.abs(want[..., 0] - (np.arange(W) + 0.5)[None, :]).max() > 0.25


@pytest.mark.parametrize("builder", [None, "gpu"], ids=["host", "device-built"])
def test_keep_current_is_set_previous(rtvk, torch, oracle, builder):
    """The previous frame kept from the context's own scene (a device to device copy of its centres,
    behind the device build when there is one) gives the plane set_previous gives; with no previous
    frame the plane is the frame's against itself, inside the snap."""
    shape = "37x19"
    W, H = SHAPES[shape][:2]
    sc, rci, prev, prev_rci, want, alone = case(oracle, shape)
    with tree_builder(builder), rtvk.Renderer(0) as r:
        M = r.motion(W, H)
        r.set_scene(sc)
        same_bits(gpu_motion(rtvk, torch, r, M, rci), alone, "no previous frame")
        r.set_scene(prev)
        M.keep_current(as_rci(rtvk, prev_rci))
        r.set_scene(sc)
        same_bits(gpu_motion(rtvk, torch, r, M, rci), want, "keep_current")
        # a frame loop: this frame becomes the next one's previous frame
        M.keep_current(as_rci(rtvk, rci))
        same_bits(gpu_motion(rtvk, torch, r, M, rci), alone, "the frame against itself")
        M.close()
    assert np.abs(alone[..., 0] - (np.arange(W) + 0.5)[None, :]).max() < SNAP
    assert np.abs(alone[..., 1] - (np.arange(H) + 0.5)[:, None]).max() < SNAP and np.all(alone[..., 3] == 1)


def test_a_changed_sphere_count_and_an_empty_scene(rtvk, torch, oracle):
    W, H = 40, 24
    sc = oracle.generate_scene(0.0)
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(f32)
    f[8:11] = [13.0, 1.0, 3.0]                   # low: the horizon crosses the frame
    f[12:15] = [-13.0, 0.5, -3.0]
    with rtvk.Renderer(0) as r:
        r.set_scene(sc)
        M = r.motion(W, H)
        M.set_previous(sc[:-1], as_rci(rtvk, rci))
        got = gpu_motion(rtvk, torch, r, M, rci)
        same_bits(got, ms.motion(oracle, sc, rci, W, H, sc[:-1], rci), "one sphere fewer")
        assert 0.1 < got[..., 3].mean() < 0.9
        M.set_previous(sc, as_rci(rtvk, rci))     # a larger previous frame: the buffer grows
        assert np.all(gpu_motion(rtvk, torch, r, M, rci)[..., 3] == 1)
        empty = np.zeros((0, 80), np.uint8)
        r.set_scene(empty)
        M.set_previous(empty, as_rci(rtvk, rci))
        got = gpu_motion(rtvk, torch, r, M, rci)
        same_bits(got, ms.motion(oracle, empty, rci, W, H), "no spheres")
        assert np.all(got[..., 3] == 1) and np.all(got[..., 2] == 0)
        M.close()


def test_refusals(rtvk, torch, renderer, oracle):
    W, H = 16, 8
    rci = as_rci(rtvk, oracle.render_call_info(1, W, H))
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    M = renderer.motion(W, H)
    renderer.render_motion(M, rci, out)
    with rtvk.Renderer(0) as other:
        other.set_scene(oracle.generate_scene(0.0))
        with other.motion(W, H) as foreign:
            with pytest.raises(rtvk.RtError) as e:
                renderer.render_motion(foreign, rci, out)
            assert e.value.code == -1 and "another context" in str(e.value)
            with pytest.raises(rtvk.RtError) as e:
                foreign.renderer = renderer          # keep_current on the wrong context
                foreign.keep_current(rci)
            assert e.value.code == -1 and "another context" in str(e.value)
            foreign.renderer = other
    with rtvk.Renderer(0) as bare:                   # no scene yet
        with bare.motion(W, H) as m2:
            for call in (lambda: bare.render_motion(m2, rci, out), lambda: m2.keep_current(rci)):
                with pytest.raises(rtvk.RtError) as e:
                    call()
                assert e.value.code == -4 and "before rt_set_scene" in str(e.value)
    lib = rtvk.load_library()
    P = ctypes.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    for args, field in (((renderer._ctx, M._state, None, P(out.data_ptr()), None, st), "rci"),
                        ((renderer._ctx, M._state, ctypes.byref(rci), None, None, st), "motion_out"),
                        ((renderer._ctx, None, ctypes.byref(rci), P(out.data_ptr()), None, st), "motion is NULL"),
                        ((None, M._state, ctypes.byref(rci), P(out.data_ptr()), None, st), "ctx")):
        assert lib.rt_render_motion_device(*args) == -1 and field.encode() in lib.rt_last_error(), field
    bad = rtvk.make_options(accel=7)
    with pytest.raises(rtvk.RtError) as e:
        renderer.render_motion(M, rci, out, options=bad)
    assert e.value.code == -1 and "accel" in str(e.value)
    zero = as_rci(rtvk, oracle.render_call_info(1, 0, H))
    with pytest.raises(rtvk.RtError) as e:
        renderer.render_motion(M, zero, out)
    assert "image_size" in str(e.value)
    M.set_previous(oracle.generate_scene(0.0), as_rci(rtvk, oracle.render_call_info(1, W, H + 1)))
    with pytest.raises(rtvk.RtError) as e:
        renderer.render_motion(M, rci, out)
    assert e.value.code == -1 and "previous" in str(e.value)
    assert lib.rt_motion_set_previous(M._state, None, 3, ctypes.byref(rci), st) == -1 and b"spheres" in lib.rt_last_error()
    assert lib.rt_motion_set_previous(M._state, None, 0, None, st) == -1 and b"prev_rci" in lib.rt_last_error()
    with pytest.raises(ValueError):
        renderer.render_motion(M, rci, torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda"))
    for w, h in ((0, 8), (8, 65536)):
        with pytest.raises(rtvk.RtError):
            renderer.motion(w, h)
    torch.cuda.synchronize()
    M.close()
    with pytest.raises(ValueError):
        renderer.render_motion(M, rci, out)
    with pytest.raises(ValueError):
        M.keep_current(rci)
    M.close()      # closing twice is harmless
