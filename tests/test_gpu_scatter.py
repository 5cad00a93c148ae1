"""One bounce of every material, the kernels' shading against the oracle's (rt_debug_scatter).

The image parity tests compare whole frames, where a texel among thousands decides whether grazing
metal, the total-internal-reflection threshold, head-on glass or a checker zero crossing is shaded
alike. This file shades given hits: Renderer.scatter_probe runs the frames' shade_rec on one lane
per case, with the sphere's records read both ways the trace kernels read them (global arrays,
the static LDS table), and every output — hit point, attenuation, raw scatter direction, next
direction, does_scatter, the LCG state afterwards — equals oracle.scatter bit for bit, floats compared
as uint32, no tolerance. scatter_cases.py holds the scenes, the case families and the float64
restatement the oracle itself is pinned to on the CPU (tests/test_oracle.py)."""
import numpy as np
import pytest

import closest_hit_cases as ch
import scatter_cases as sc
from test_gpu_parity import tree_builder

pytestmark = pytest.mark.gpu

BUILDER = {"materials": None, "device17": "gpu"}
OUTPUTS = ("p", "att", "sd", "d_next", "scatter", "seed")
FORM_NAME = {0: "global", 1: "lds-rec"}


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
    """One renderer, the scene it holds, and every scene's cases with the oracle's answers, computed
    once and never changed."""

    def __init__(self, rtvk, oracle):
        self.rtvk, self.oracle = rtvk, oracle
        self.renderer = rtvk.Renderer(0)
        self.current, self.memo = None, {}

    def cases(self, name):
        if name not in self.memo:
            scene, fams = sc.all_cases(self.oracle, name)
            ref = {}
            for fam, args in fams.items():
                ref[fam] = self.oracle.scatter(scene, *args)
                for a in ref[fam].values():
                    a.setflags(write=False)
            self.memo[name] = (scene, fams, ref)
        return self.memo[name]

    def use(self, name):
        scene = self.cases(name)[0]
        if self.current != name:
            with tree_builder(BUILDER[name]):
                self.renderer.set_scene(np.ascontiguousarray(scene, np.uint8).reshape(-1, 80))
            self.current = name
            assert self.renderer.scene_array(8)["device_built"] == (BUILDER[name] == "gpu")
        return scene


@pytest.fixture(scope="module")
def bench(rtvk, oracle):
    b = Bench(rtvk, oracle)
    yield b
    b.renderer.close()


def assert_bits(what, got, ref, args):
    """All six outputs of every case, as 32-bit words."""
    rays, ids, t, seeds = args
    for name in OUTPUTS:
        g, r = np.ascontiguousarray(got[name]).view(np.uint32), np.ascontiguousarray(ref[name]).view(np.uint32)
        bad = np.flatnonzero((g != r).reshape(len(ids), -1).any(axis=1))
        lines = [f"case {int(i)} ray={rays[i].tolist()} id={int(ids[i])} t={float(t[i])!r} seed={int(seeds[i])}: {name} "
                 f"{got[name][i].tolist()}; oracle {ref[name][i].tolist()}" for i in bad[:4]]
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {len(ids)} cases:\n" + "\n".join(lines)


@pytest.mark.parametrize("form", [0, 1], ids=[FORM_NAME[0], FORM_NAME[1]])
@pytest.mark.parametrize("scene", sc.SCENES)
def test_scatter_equals_oracle(bench, scene, form):
    """Both scenes (host-built records from make_mat on the host; device-built ones from the
    device's), both record forms, every family, head_on included: all six outputs bit for bit."""
    bench.use(scene)
    _, fams, ref = bench.cases(scene)
    for fam in sc.FAMILIES:
        got = bench.renderer.scatter_probe(*fams[fam], form=form)
        assert_bits(f"{scene} {FORM_NAME[form]} {fam}", got, ref[fam], fams[fam])


def test_families_reach_their_materials(bench):
    """The cases are what they are for: every material and texture id of the palette is shaded in
    the generic family, with and without a scatter, with 0, 1 and 3 draws; the head-on family holds
    dielectrics that take no draw."""
    for scene in sc.SCENES:
        sce, fams, ref = bench.cases(scene)
        R = sc.records(sce)
        _, ids, _, seeds = fams["generic"]
        kinds = {(int(m), int(x)) for m, x in zip(R["mtype"][ids], R["ttype"][ids])}
        assert {(m, x) for m, x, _ in sc.PALETTE} <= kinds
        assert (ref["generic"]["scatter"] == 0).sum() > 200 and (ref["generic"]["scatter"] == 1).sum() > 10000
        s1 = sc.lcg(seeds.astype(np.uint64))
        s3 = sc.lcg(sc.lcg(s1))
        after = ref["generic"]["seed"]
        assert (after == seeds).sum() > 100 and (after == s1).sum() > 1000 and (after == s3).sum() > 1000
        _, hid, _, hseeds = fams["head_on"]
        assert (ref["head_on"]["seed"] == hseeds).sum() > 100


@pytest.mark.parametrize("form", [0, 1], ids=[FORM_NAME[0], FORM_NAME[1]])
def test_ragged_batches(bench, form):
    """Batches that end inside a wave and inside the 256-thread block: n = 1, 63, 64, 65, 257, 4097."""
    bench.use("materials")
    _, fams, ref = bench.cases("materials")
    args = fams["bounce"]
    for n in (1, 63, 64, 65, 257, 4097):
        got = bench.renderer.scatter_probe(*(a[:n] for a in args), form=form)
        assert_bits(f"n = {n}", got, {k: v[:n] for k, v in ref["bounce"].items()}, tuple(a[:n] for a in args))


@pytest.mark.parametrize("form", [0, 1], ids=[FORM_NAME[0], FORM_NAME[1]])
def test_probe_sees_what_a_frame_sees(bench, rtvk, oracle, form):
    """A 24x16 one-sample depth-2 STREAM frame of the material scene, taken apart: the camera rays
    (shader.rgen:56-58, 107-115 restated with numpy in binary32, four draws each) go through
    closest_hits, scatter_probe, closest_hits and scatter_probe again, the second segment traced
    along the first bounce's raw scatter direction as a frame traces it; the colour put together from
    the probes' answers (shader.rgen:70-89) is the oracle's frame colour in every pixel."""
    W, H = 24, 16
    scene = bench.use("materials")
    r = bench.renderer
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(np.float32)
    f[8:11] = [7.0, 1.6, 2.0]        # a low, near camera: spheres, ground and sky all in the frame
    f[12:15] = [-7.0, -1.2, -2.0]
    acc, _, _ = oracle.render(scene, rci, W, H, opts=oracle.options(max_depth=2))
    vp = np.zeros(18, np.float32)
    oracle.lib().orc_viewport(rci.ctypes.data, vp.ctypes.data)
    look_from, hor, ver, ulc = vp[0:3], vp[3:6], vp[6:9], vp[9:12]
    rays = np.zeros((H * W, 6), np.float32)
    seeds = np.zeros(H * W, np.uint64)
    for y in range(H):
        for x in range(W):
            s = oracle.pixel_seed(x, y)
            r0, r1 = oracle.random_floats(s, 2)
            ux = (np.float32(x) + np.float32(r0)) / np.float32(W)
            uy = (np.float32(y) + np.float32(r1)) / np.float32(H)
            to = (ulc + ux * hor) - uy * ver
            rays[y * W + x] = np.concatenate([look_from, to - look_from])
            seeds[y * W + x] = s
    for _ in range(4):                # uv.x, uv.y and the lens disk's two
        seeds = sc.lcg(seeds)
    seeds = seeds.astype(np.uint32)
    sky = np.float32([0.7, 0.8, 1.0])
    colour = np.tile(sky, (H * W, 1))
    ids1, t1 = r.closest_hits(rays)
    h1 = np.flatnonzero(ids1 != ch.MISS)
    b1 = r.scatter_probe(rays[h1], ids1[h1], t1[h1], seeds[h1], form=form)
    colour[h1] = b1["att"]                                       # absorbed: light = attenuation
    go = b1["scatter"] == 1
    rays2 = np.concatenate([b1["p"][go], b1["sd"][go]], axis=1)
    ids2, t2 = r.closest_hits(rays2)
    colour[h1[go]] = b1["att"][go] * sky                         # second segment misses
    h2 = np.flatnonzero(ids2 != ch.MISS)
    b2 = r.scatter_probe(rays2[h2], ids2[h2], t2[h2], b1["seed"][go][h2], form=form)
    second = np.where((b2["scatter"] == 1)[:, None], np.float32(0.0), b2["att"])   # depth exhausted: light stays 0
    colour[h1[go][h2]] = (b1["att"][go][h2] * second).astype(np.float32)
    np.testing.assert_array_equal(colour.reshape(H, W, 3), acc[..., :3])
    assert len(h1) > 100 and len(h1) < H * W and go.sum() > 50 and (~go).sum() >= 1 and len(h2) > 20
    assert (b2["scatter"] == 0).sum() >= 1


def test_probe_between_frames_changes_nothing(bench, rtvk, torch, oracle):
    """The probe goes through no launch plan: between two frames of a context it leaves the images,
    the tile-cost record, the hand-out order and the launch report alone."""
    W, H = 96, 64
    scene = bench.use("materials")
    r = bench.renderer
    rci_np = oracle.render_call_info(3, W, H)
    rci = rtvk.RenderCallInfo.from_buffer_copy(rci_np.tobytes())
    ref_acc, ref_out, _ = oracle.render(scene, rci_np, W, H)

    def frame():
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        r.render_device(rci, acc, out)
        torch.cuda.synchronize()
        return acc.cpu().numpy(), out.cpu().numpy()

    a0, o0 = frame()
    cost0 = r.tile_costs().copy()
    plan0 = r.launch_info()
    _, fams, ref = bench.cases("materials")
    args = tuple(a[:5000] for a in fams["generic"])
    for form in (0, 1):
        assert_bits("between frames", r.scatter_probe(*args, form=form), {k: v[:5000] for k, v in ref["generic"].items()}, args)
    assert r.launch_info() == plan0
    np.testing.assert_array_equal(r.tile_costs(), cost0)
    a1, o1 = frame()
    assert r.launch_info()["form"] == plan0["form"]
    for a, o in ((a0, o0), (a1, o1)):
        np.testing.assert_array_equal(a, ref_acc)
        np.testing.assert_array_equal(o, ref_out)
    assert cost0.size == (W // 8) * (H // 8) and cost0.max() > 0


def test_arguments(bench, rtvk, oracle):
    """n = 0 is an empty success. A non-finite ray value or t, a direction without a nonzero
    component, a sphere index beyond the scene, an unknown form, NULL arrays and the LDS form on a
    scene of more than 512 spheres are refused with RT_ERR_INVALID_ARGUMENT, a call before
    rt_set_scene with RT_ERR_NO_SCENE."""
    bench.use("materials")
    r = bench.renderer
    rays, ids, t, seeds = (a[:70].copy() for a in bench.cases("materials")[1]["generic"])
    out = r.scatter_probe(rays[:0], ids[:0], t[:0], seeds[:0])
    assert all(out[k].shape[0] == 0 for k in OUTPUTS)

    def refused(code, *args, **kw):
        with pytest.raises(rtvk.RtError) as e:
            r.scatter_probe(*args, **kw)
        assert e.value.code == code, e.value
        return str(e.value)

    for k, v in [(0, np.nan), (2, np.inf), (4, -np.inf), (3, np.nan)]:
        bad = rays.copy()
        bad[65, k] = v
        assert "case 65" in refused(-1, bad, ids, t, seeds)
    bad = rays.copy()
    bad[3, 3:] = [0.0, -0.0, 0.0]
    assert "case 3" in refused(-1, bad, ids, t, seeds)
    for v in (np.nan, np.inf):
        bad = t.copy()
        bad[7] = v
        assert "case 7" in refused(-1, rays, ids, bad, seeds)
    for v in (488, 0xFFFFFFFF):
        bad = ids.copy()
        bad[69] = v
        assert "case 69" in refused(-1, rays, bad, t, seeds)
    refused(-1, rays, ids, t, seeds, form=2)
    lib = rtvk.load_library()
    z = np.zeros(16, np.float32)
    p = z.ctypes.data
    assert lib.rt_debug_scatter(r._ctx, None, p, p, p, 1, 0, p, p, p, p, p, p) == -1
    assert lib.rt_debug_scatter(r._ctx, p, p, p, p, 1, 0, p, p, None, p, p, p) == -1
    assert lib.rt_debug_scatter(None, p, p, p, p, 1, 0, p, p, p, p, p, p) == -1
    assert lib.rt_debug_scatter(r._ctx, p, p, p, p, (1 << 24) + 1, 0, p, p, p, p, p, p) == -1   # refused before any read
    with rtvk.Renderer(0) as other:
        with pytest.raises(rtvk.RtError) as e:
            other.scatter_probe(rays, ids, t, seeds)
        assert e.value.code == -4
        big = oracle.generate_scene(0.0, 12)          # 580 spheres: beyond the static LDS table
        other.set_scene(big)
        with pytest.raises(rtvk.RtError) as e:
            other.scatter_probe(rays, ids, t, seeds, form=1)
        assert e.value.code == -1
        ref = oracle.scatter(big, rays, ids, t, seeds)
        assert_bits("580 spheres, global records", other.scatter_probe(rays, ids, t, seeds, form=0), ref, (rays, ids, t, seeds))
