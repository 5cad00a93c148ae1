"""First-hit feature buffers (rt_render_features_device), every walk form against
the numpy restatement (tests/denoise_sim.py), bit for bit: the camera rays of the counter-based
stream, their closest hits by the production kernels' MODE_FEATURES instantiation, the albedo, the
oriented normal and the depth by the shading's expressions, summed in binary32 in sample order.
Shapes are the smallest that hold more than one 8x8 tile, more than one 64-unit block and partial
tiles at the right and bottom edges; the restatement of a geometry is computed once at the largest
sample count and shared (a smaller count is a prefix of the same per-sample values)."""
import numpy as np
import pytest

import denoise_sim as ds
from test_gpu_closest_hit import FORM_NAME, PROBE_FORMS, REGATE
from test_gpu_parity import BRUTE, HASH, LBVH, STREAM, WALK_FORM, tree_builder

pytestmark = pytest.mark.gpu

F_MAX = 16
COUNTS = (1, 3, 16)
SHAPES = ((40, 24), (37, 19))


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


class Bench:
    """One renderer and the scene it currently holds (set again only when it changes)."""

    def __init__(self, rtvk, torch):
        self.rtvk, self.torch = rtvk, torch
        self.renderer = rtvk.Renderer(0)
        self.current = None

    def use(self, key, scene, builder=None):
        if self.current != (key, builder):
            with tree_builder(builder):
                self.renderer.set_scene(np.ascontiguousarray(scene, np.uint8).reshape(-1, 80))
            self.current = (key, builder)

    def options(self, form=LBVH, **kw):
        o = self.rtvk.make_options(accel=BRUTE if form == BRUTE else LBVH, rng_mode=HASH, **kw)
        o.reserved[1] = WALK_FORM.get(form, 0)
        if form == REGATE:
            o.reserved[0] |= 2
        return o

    def features(self, rci_np, W, H, F, options, rows=None):
        t = self.torch
        rci = self.rtvk.RenderCallInfo.from_buffer_copy(np.ascontiguousarray(rci_np).tobytes())
        f0 = t.full((H, W, 4), -7.0, dtype=t.float32, device="cuda")
        f1 = t.full((H, W, 4), -7.0, dtype=t.float32, device="cuda")
        rows_t = None if rows is None else t.tensor(np.asarray(rows, np.int32), device="cuda")
        self.renderer.render_features(rci, f0, f1, samples=F, rows=rows_t, options=options)
        t.cuda.synchronize()
        return f0.cpu().numpy(), f1.cpu().numpy()


@pytest.fixture(scope="module")
def bench(rtvk, torch):
    b = Bench(rtvk, torch)
    yield b
    b.renderer.close()


def assert_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check(bench, oracle, scene, rci_np, W, H, options, what, counts=COUNTS, **kw):
    vals = ds.values(oracle, scene, rci_np, W, H, max(counts), sample_base=int(options.sample_base),
                     seed_local=bool(options.seed_mode), **kw)
    for F in counts:
        f0, f1 = bench.features(rci_np, W, H, F, options, rows=kw.get("rows"))
        r0, r1 = ds.sum_samples(vals, F)
        assert_bits(f0, r0, (what, F, "feat0"))
        assert_bits(f1, r1, (what, F, "feat1"))
    return vals


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("builder", [None, "gpu"])
@pytest.mark.parametrize("form", PROBE_FORMS, ids=lambda f: FORM_NAME[f])
def test_every_form_matches_the_restatement(bench, oracle, form, builder, shape):
    W, H = shape
    sc = oracle.generate_scene()
    bench.use("canon", sc, builder)
    vals = check(bench, oracle, sc, oracle.render_call_info(1, W, H), W, H, bench.options(form), FORM_NAME[form])
    assert bench.renderer.launch_info()["chunks"] == 1       # one unit per pixel: the sums' order
    hit = vals[..., 3]
    assert 0.5 < hit.mean() <= 1.0 and np.unique(vals[..., 0:3].reshape(-1, 3), axis=0).shape[0] > 20


def low_camera(oracle, W, H):
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(np.float32)
    f[8:11] = [13.0, 1.0, 3.0]
    f[12:15] = [-13.0, 0.5, -3.0]
    return rci


def test_horizon_crosses_the_frame(bench, oracle):
    sc = oracle.generate_scene()
    bench.use("canon", sc)
    vals = check(bench, oracle, sc, low_camera(oracle, 40, 24), 40, 24, bench.options(), "low camera")
    miss = vals[..., 3] == 0
    assert 0.1 < miss.mean() < 0.9
    assert np.all(vals[miss][:, 0:3] == np.float32(ds.SKY)) and np.all(vals[miss][:, 4:8] == 0)


def test_camera_inside_a_dielectric_sphere(bench, oracle):
    """Every ray starts inside the radius-1 glass sphere at (0, 1, 0) and hits it from inside: back
    faces, n = -outward (it points at the camera's side), depth below the diameter."""
    sc = oracle.generate_scene()
    geo = np.ascontiguousarray(sc[:, :16]).view(np.float32).reshape(-1, 4)
    mtype = np.ascontiguousarray(sc[:, 16:20]).view(np.uint32).reshape(-1)
    glass = int(np.flatnonzero((geo[:, 3] == 1.0) & (mtype == 2))[0])
    c = geo[glass, :3]
    rci = oracle.render_call_info(1, 40, 24)
    f = rci.view(np.float32)
    f[8:11] = c + np.float32([0.2, 0.1, 0.3])
    f[12:15] = [1.0, -0.2, 0.5]
    bench.use("canon", sc)
    vals = check(bench, oracle, sc, rci, 40, 24, bench.options(), "inside glass")
    assert np.all(vals[..., 3] == 1) and np.all(vals[..., 7] < 2.0)
    rays = ds.camera_rays(oracle, rci, 40, 24, 1)[:, :, 0]
    d = rays[..., 3:6] / np.linalg.norm(rays[..., 3:6], axis=-1, keepdims=True)
    assert np.all(np.sum(vals[:, :, 0, 4:7] * d, axis=-1) < 0)      # the oriented normal faces the ray


def test_checkered_small_spheres(bench, oracle):
    sc = oracle.generate_scene().copy()
    small = np.arange(4, sc.shape[0], 3)
    sc[small, 20:24] = np.frombuffer(np.uint32(1).tobytes(), np.uint8)      # textureType = CHECKERED
    col1 = np.ascontiguousarray(sc[small, 48:64]).view(np.float32).reshape(-1, 4)
    col1[:] = [0.9, 0.1, 0.2, 0.0]
    sc[small, 48:64] = col1.view(np.uint8).reshape(-1, 16)
    bench.use("checkered", sc)
    vals = check(bench, oracle, sc, oracle.render_call_info(1, 40, 24), 40, 24, bench.options(), "checkered spheres")
    red = np.all(vals[..., 0:3] == np.float32([0.9, 0.1, 0.2]), axis=-1)
    assert red.sum() > 20                                            # the second colour is seen


def test_rows_offset_seed_mode_and_sample_base(bench, oracle):
    sc = oracle.generate_scene()
    bench.use("canon", sc)
    W, H = 40, 24
    # every second row of a taller, wider image, from a nonzero offset
    rci = oracle.render_call_info(1, 96, 64, offset=(8, 0))
    rows = 3 + 2 * np.arange(H)
    check(bench, oracle, sc, rci, W, H, bench.options(), "rows", counts=(3,), rows=rows)
    # launch-local seeds on an offset band differ from the global ones and match their restatement
    rci = oracle.render_call_info(1, 96, 64, offset=(8, 4), number=2)
    v_local = check(bench, oracle, sc, rci, W, H, bench.options(seed_mode=1), "launch-local seeds", counts=(3,))
    v_global = check(bench, oracle, sc, rci, W, H, bench.options(), "global seeds", counts=(3,))
    assert not np.array_equal(v_local, v_global)
    # sample_base: samples [5, 8) are the tail of samples [0, 8)
    v5 = check(bench, oracle, sc, oracle.render_call_info(1, W, H), W, H, bench.options(sample_base=5), "sample_base",
               counts=(3,))
    v0 = ds.values(oracle, sc, oracle.render_call_info(1, W, H), W, H, 8)
    np.testing.assert_array_equal(v5, v0[:, :, 5:8])


def test_empty_scene(bench, oracle):
    sc = np.zeros((0, 80), np.uint8)
    bench.use("empty", sc)
    for form in (LBVH, BRUTE):
        f0, f1 = bench.features(oracle.render_call_info(1, 37, 19), 37, 19, 3, bench.options(form))
        want = np.float32(ds.SKY) + np.float32(ds.SKY) + np.float32(ds.SKY)
        assert np.all(f0[..., 0:3] == want) and np.all(f0[..., 3] == 0) and np.all(f1 == 0)


def test_refusals(bench, rtvk, torch, oracle):
    bench.use("canon", oracle.generate_scene())
    rci = oracle.render_call_info(1, 16, 8)
    cases = [(bench.rtvk.make_options(rng_mode=STREAM), 4), (bench.options(accumulate=True), 4), (bench.options(), 0),
             (bench.options(), 257)]
    for options, F in cases:
        with pytest.raises(rtvk.RtError) as e:
            bench.features(rci, 16, 8, F, options)
        assert e.value.code == -1
    bench.features(rci, 16, 8, 256, bench.options())              # the largest count is accepted


@pytest.mark.parametrize("rng_mode", [STREAM, HASH])
def test_features_between_frames_change_nothing(bench, rtvk, torch, oracle, rng_mode):
    """Render, features, render gives the oracle's image twice; the second frame runs in the tile
    order of the first, whose tile-cost record the features launch left untouched."""
    W, H = 96, 64
    sc = oracle.generate_scene()
    bench.use("canon", sc)
    r = bench.renderer
    rci_np = oracle.render_call_info(3, W, H)
    rci = rtvk.RenderCallInfo.from_buffer_copy(rci_np.tobytes())
    ref_acc, ref_out, _ = oracle.render(sc, rci_np, W, H, opts=oracle.options(rng_mode=rng_mode))

    def frame():
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        r.render_device(rci, acc, out, options=rtvk.make_options(rng_mode=rng_mode))
        torch.cuda.synchronize()
        return acc.cpu().numpy(), out.cpu().numpy()

    a0, o0 = frame()
    cost0 = r.tile_costs().copy()
    plan0 = r.launch_info()
    waits0 = r.host_waits()
    f0, f1 = bench.features(rci_np, W, H, 4, bench.options())
    r0, r1 = ds.features(oracle, sc, rci_np, W, H, 4)
    assert_bits(f0, r0, "feat0")
    assert_bits(f1, r1, "feat1")
    assert r.launch_info()["chunks"] == 1 and r.host_waits() == waits0
    np.testing.assert_array_equal(r.tile_costs(), cost0)
    a1, o1 = frame()
    assert r.launch_info()["form"] == plan0["form"]
    for a, o in ((a0, o0), (a1, o1)):
        np.testing.assert_array_equal(a, ref_acc)
        np.testing.assert_array_equal(o, ref_out)
    assert cost0.size == (W // 8) * (H // 8) and cost0.max() > 0
