"""The closest hit of single rays, every walk form against the oracle (rt_debug_closest_hits).

The image parity tests prove the whole chain for the rays a camera and a random walk happen to
produce. This file probes the operation underneath — closest hit, lowest index on ties — with rays
chosen to sit on the edges the exactness arguments of DESIGN.md §4.3 and §4.6 were written for:
sphere surfaces, zero and denormal direction components, cell planes and cell diagonals, grazing
rays whose discriminant and AABB gate are decided by rounding, and origins beyond the pad radius
with hits at tmax. The probe runs the production kernels (MODE_PROBE: a ray per unit), the
comparator is oracle.closest_hits (bit-exact: the id, and the bits of t wherever there is a hit);
closest_hit_cases.py holds the scenes, the families and the float64 reference the oracle itself is
checked against on the CPU (tests/test_oracle.py)."""
import numpy as np
import pytest

import closest_hit_cases as ch
from test_gpu_parity import BRUTE, FORMS, GRID, GRID_COOP, GRID_CQ, LBVH, LBVH_GLOBAL, LBVH_LDS1, LBVH_OCT, WALK_FORM
from test_gpu_parity import tree_builder

pytestmark = pytest.mark.gpu

REGATE = "regate"     # the default form with every winner recomputed by regate_brute (force_regate)
PROBE_FORMS = FORMS + [GRID, REGATE]
FORM_NAME = {BRUTE: "brute", LBVH: "default", LBVH_OCT: "oct", LBVH_LDS1: "lds1", LBVH_GLOBAL: "global",
             GRID: "grid", GRID_COOP: "coop", GRID_CQ: "cq", REGATE: "regate"}
CASES = [(s, b) for s in ch.SCENES for b in (None, "gpu")] + [("big", "gpu")]

# The kernel form (rt_debug_launch_info) each requested form runs as: the launch plan's choice
# (choose_accel). Host-built scenes stage their grid and trees in LDS and walk the grid by default;
# device-built small scenes walk the octant tree by default and read their grid from L2 when one is
# asked for; `big` (6 404 spheres, device-built) reads grid and tree from L2 and has the treelet.
NEAR = {
    "host": {BRUTE: "brute", LBVH: "grid-lds-rec", LBVH_OCT: "lbvh-octant-lds", LBVH_LDS1: "lbvh-lds",
             LBVH_GLOBAL: "lbvh-global", GRID: "grid-lds-rec", GRID_COOP: "grid-lds-coop", GRID_CQ: "grid-lds-rec-cq",
             REGATE: "grid-lds-rec"},
    "gpu": {BRUTE: "brute", LBVH: "lbvh-octant-lds", LBVH_OCT: "lbvh-octant-lds", LBVH_LDS1: "lbvh-lds",
            LBVH_GLOBAL: "lbvh-global", GRID: "grid-global", GRID_COOP: "grid-global-coop", GRID_CQ: "grid-global",
            REGATE: "lbvh-octant-lds"},
    "big": {BRUTE: "brute", LBVH: "grid-global", LBVH_OCT: "lbvh-treelet", LBVH_LDS1: "lbvh-treelet",
            LBVH_GLOBAL: "lbvh-global", GRID: "grid-global", GRID_COOP: "grid-global-coop", GRID_CQ: "grid-global",
            REGATE: "grid-global"},
}
# an origin beyond the grid's pad radius (the `far` family): the plan refuses the grid, and the
# forms that asked for it fall back to a tree (the default's, or for an explicit grid form the tree
# from L2 / the treelet)
FAR = {
    "host": {**NEAR["host"], LBVH: "lbvh-octant-lds", REGATE: "lbvh-octant-lds", GRID: "lbvh-global",
             GRID_COOP: "lbvh-global", GRID_CQ: "lbvh-global"},
    "gpu": {**NEAR["gpu"], GRID: "lbvh-treelet", GRID_COOP: "lbvh-treelet", GRID_CQ: "lbvh-treelet"},
    "big": {**NEAR["big"], LBVH: "lbvh-treelet", REGATE: "lbvh-treelet", GRID: "lbvh-treelet",
            GRID_COOP: "lbvh-treelet", GRID_CQ: "lbvh-treelet"},
}
FLAT_SCENES = ("canon", "lattice", "big")      # their grids are one cell thick in y
FLAT_FORMS = ("grid-lds", "grid-lds-rec", "grid-global")


def expected_form(scene, builder, form, family):
    """(kernel form, one-layer grid walk) the launch must report."""
    kind = "big" if scene == "big" else (builder or "host")
    name = (FAR if family == "far" else NEAR)[kind][form]
    return name, scene in FLAT_SCENES and name in FLAT_FORMS


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
    """One renderer, the scene it currently holds, and every (scene, family)'s rays and oracle
    answers, computed once and never changed. A batch with an origin beyond the scene's pad radius
    makes the context re-pad its node boxes for it, as a far camera does, and the wider boxes stay
    until the next set_scene: after such a probe the scene is set again before anything else runs,
    so every other case walks the tree at the padding its build gave it, whatever ran before."""

    def __init__(self, rtvk, oracle):
        self.rtvk, self.oracle = rtvk, oracle
        self.renderer = rtvk.Renderer(0)
        self.current, self.pad_radius = None, 0.0
        self.scenes, self.layouts, self.memo = {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = ch.make_scene(self.oracle, name)
        return self.scenes[name]

    def use(self, name, builder):
        if self.current != (name, builder):
            with tree_builder(builder):
                self.renderer.set_scene(np.ascontiguousarray(self.scene(name), np.uint8).reshape(-1, 80))
            self.current = (name, builder)
            self.pad_radius = self.renderer.scene_array(8)["scene_radius"] * 1.01 + 100.0   # rt_set_scene's
        if (name, builder) not in self.layouts:
            r = self.renderer
            grid = r.scene_array(9)
            self.layouts[(name, builder)] = None if grid["cells"] == 0 else ch.grid_layout(
                ch.geometry(self.scene(name)), grid["n"], r.scene_array(8)["scene_radius"], r.scene_array(3))
        return self.layouts[(name, builder)]

    def family(self, name, builder, fam):
        """(rays, oracle ids, oracle t) of a family; the families that are laid on the grid's planes
        (axis, boundary) belong to a builder's grid, the others to the scene."""
        layout = self.use(name, builder)
        key = (name, fam, builder if fam in ("axis", "boundary") else None)
        if key not in self.memo:
            if fam == "bounce":
                self.family(name, builder, "generic")
            n = ch.N_RAYS_BIG if name == "big" else ch.N_RAYS
            rays = ch.family(self.oracle, self.scene(name), fam, layout, n, {"generic": self.memo.get((name, "generic", None))})
            ids, t = self.oracle.closest_hits(self.scene(name), rays)
            for a in (rays, ids, t):
                a.setflags(write=False)
            self.memo[key] = (rays, ids, t)
        return self.memo[key]

    def options(self, form):
        o = self.rtvk.make_options(accel=BRUTE if form == BRUTE else LBVH)
        o.reserved[1] = WALK_FORM.get(form, 0)
        if form == REGATE:
            o.reserved[0] |= 2
        return o

    def probe(self, rays, form):
        far = len(rays) and float(np.linalg.norm(np.asarray(rays, np.float64)[:, :3], axis=1).max()) > 0.99 * self.pad_radius
        try:
            return self.renderer.closest_hits(rays, options=self.options(form))
        finally:
            if far:
                self.current = None   # re-padded: use() sets the scene again


@pytest.fixture(scope="module")
def bench(rtvk, oracle):
    b = Bench(rtvk, oracle)
    yield b
    b.renderer.close()


def assert_hits(form, rays, ids, t, ref_ids, ref_t):
    """The winner of every ray, and the bits of its t wherever there is one."""
    hit = ref_ids != ch.MISS
    bad = np.flatnonzero((ids != ref_ids) | (hit & (t.view(np.uint32) != ref_t.view(np.uint32))))
    lines = [f"ray {int(i)} o={rays[i, :3].tolist()} v={rays[i, 3:].tolist()}: form {FORM_NAME[form]} id {int(ids[i])} "
             f"t {float(t[i])!r}; oracle id {int(ref_ids[i])} t {float(ref_t[i])!r}" for i in bad[:6]]
    assert bad.size == 0, f"{bad.size} of {len(rays)} rays differ:\n" + "\n".join(lines)


@pytest.mark.parametrize("family", ch.FAMILIES)
@pytest.mark.parametrize("form", PROBE_FORMS, ids=[FORM_NAME[f] for f in PROBE_FORMS])
@pytest.mark.parametrize("scene,builder", CASES, ids=[f"{s}-{b or 'host'}" for s, b in CASES])
def test_closest_hit_equals_oracle(bench, scene, builder, form, family):
    """For every scene, builder, walk form and ray family: the probe's winner equals the oracle's
    for every ray, and so do the bits of t wherever a sphere is hit; the form that ran is the form
    asked for (or, beyond the grid's pad radius, the plan's fallback)."""
    rays, ref_ids, ref_t = bench.family(scene, builder, family)
    ids, t = bench.probe(rays, form)
    info = bench.renderer.launch_info()
    assert (info["form"], info["flat_grid"]) == expected_form(scene, builder, form, family), info
    assert_hits(form, rays, ids, t, ref_ids, ref_t)


@pytest.mark.parametrize("builder", [None, "gpu"])
def test_denormal_direction_regression(bench, builder):
    """The ray this probe caught (closest_hit_cases.DENORMAL_RAY on `cloud`): a direction component
    that normalises to a denormal has a finite reciprocal of 2.3e38, and the tree walks' node test
    computed o / d as inf and culled every box (they reported a miss; node_inv now clamps every
    reciprocal beyond 2^100). Every form reports the oracle's sphere 22 at its t, also with the
    component moved to each axis and sign."""
    bench.use("cloud", builder)
    rays = []
    for shift in range(3):
        for sign in (1.0, -1.0):
            r = ch.DENORMAL_RAY.copy()
            r[4] *= np.float32(sign)
            rays.append(np.concatenate([np.roll(r[:3], shift), np.roll(r[3:], shift)]))
    rays = np.asarray(rays, np.float32)
    ref_ids, ref_t = bench.oracle.closest_hits(bench.scene("cloud"), rays)
    assert ref_ids[0] == 22 and ref_t[0] == np.float32(0.028013616800308228)
    for form in PROBE_FORMS:
        ids, t = bench.probe(rays, form)
        assert_hits(form, rays, ids, t, ref_ids, ref_t)


@pytest.mark.parametrize("scene,builder", CASES, ids=[f"{s}-{b or 'host'}" for s, b in CASES])
def test_families_reach_their_edges(bench, scene, builder):
    """What the families are for, checked on their own inputs with the oracle: the generic family
    hits and misses, the bounce family starts on surfaces (hits within 1e-2 of tmin are there), the
    tangent family holds rounding corners (a winner of the quadratic that fails the AABB gate), the
    far family has hits on both sides of tmax's neighbourhood, reports accepted at exactly tmax and
    reports of exactly its successor, which are refused."""
    sc = bench.scene(scene)
    _, gi, _ = bench.family(scene, builder, "generic")
    assert 0.3 < (gi != ch.MISS).mean() < 0.95
    rays, bi, bt = bench.family(scene, builder, "bounce")
    assert ((bi != ch.MISS) & (bt < 1e-2)).sum() >= 32
    rays, ti, _ = bench.family(scene, builder, "tangent")
    ui, _ = bench.oracle.closest_hits(sc, rays, gated=False)
    assert ((ui != ti) & (ui != ch.MISS)).sum() >= 32
    rays, fi, ft = bench.family(scene, builder, "far")
    assert ((fi != ch.MISS) & (ft > 9990.0)).sum() >= 32 and (fi == ch.MISS).sum() >= 32
    accepted, refused = ch.tmax_edge_counts(bench.oracle, sc, rays, fi, ft)
    assert accepted >= 4 and refused >= 4, (accepted, refused)   # t exactly tmax, and exactly its successor
    for fam in ("axis", "boundary"):
        assert bench.family(scene, builder, fam)[1].size >= (ch.N_RAYS_BIG if scene == "big" else ch.N_RAYS)


@pytest.mark.parametrize("form", PROBE_FORMS, ids=[FORM_NAME[f] for f in PROBE_FORMS])
def test_ragged_batches(bench, form):
    """Batches that end inside a wave, a block and a band row: n = 1, 63, 64, 65, 64 k + 1 and one
    ray past a band row (513) and past the 768-thread block (769)."""
    rays, ref_ids, ref_t = bench.family("canon", None, "generic")
    for n in (1, 63, 64, 65, 64 * 7 + 1, 513, 769, 4097):
        ids, t = bench.probe(rays[:n], form)
        assert_hits(form, rays[:n], ids, t, ref_ids[:n], ref_t[:n])


@pytest.mark.parametrize("scene,builder", [("nobig", None), ("nobig", "gpu"), ("manybig", None), ("manybig", "gpu")])
def test_big_sphere_groups(bench, scene, builder):
    """A scene with no big sphere (the segment's four unconditional table records are inert) and one
    with eight (the further groups' loop), every form."""
    bench.use(scene, builder)
    n_big = bench.renderer.scene_array(8)["n_big"]
    assert n_big == 0 if scene == "nobig" else n_big > 4
    rays = ch.generic(ch.geometry(bench.scene(scene)), 1 << 13)
    ref_ids, ref_t = bench.oracle.closest_hits(bench.scene(scene), rays)
    assert 0.1 < (ref_ids != ch.MISS).mean() < 0.95
    for form in PROBE_FORMS:
        ids, t = bench.probe(rays, form)
        assert_hits(form, rays, ids, t, ref_ids, ref_t)


def test_empty_scene_and_arguments(bench, rtvk):
    """An empty scene misses everywhere in every form. n = 0 is an empty success; a non-finite
    value, an all-zero direction and an unknown accel are refused, and so is a call before
    rt_set_scene."""
    rays, _, _ = bench.family("canon", None, "generic")
    r = bench.renderer
    r.set_scene(np.zeros((0, 80), np.uint8))
    bench.current = None
    for form in PROBE_FORMS:
        ids, _ = bench.probe(rays[:1000], form)
        assert np.all(ids == ch.MISS), FORM_NAME[form]
    ids, t = r.closest_hits(np.zeros((0, 6), np.float32))
    assert ids.shape == (0,) and t.shape == (0,)
    for k, v in [(0, np.nan), (2, np.inf), (4, -np.inf), (3, np.nan)]:
        bad = rays[:70].copy()
        bad[65, k] = v
        with pytest.raises(rtvk.RtError) as e:
            r.closest_hits(bad)
        assert e.value.code == -1 and "ray 65" in str(e.value)
    bad = rays[:70].copy()
    bad[3, 3:] = [0.0, -0.0, 0.0]
    with pytest.raises(rtvk.RtError) as e:
        r.closest_hits(bad)
    assert e.value.code == -1 and "ray 3" in str(e.value)
    o = rtvk.make_options(accel=3)
    with pytest.raises(rtvk.RtError) as e:
        r.closest_hits(rays[:8], options=o)
    assert e.value.code == -1
    with rtvk.Renderer(0) as fresh:
        with pytest.raises(rtvk.RtError) as e:
            fresh.closest_hits(rays[:8])
        assert e.value.code == -4


@pytest.mark.parametrize("rng_mode", [0, 2])
def test_probe_between_frames_changes_nothing(bench, rtvk, torch, oracle, rng_mode):
    """A probe between two frames of a context leaves them alone: render, probe, render gives the
    oracle's image twice, the second frame runs in the LPT order of the first (its tile-cost record
    is the one the first frame left, untouched by the probe), and the probe's own answers are the
    oracle's."""
    W, H = 96, 64
    bench.use("canon", None)
    r = bench.renderer
    rci_np = oracle.render_call_info(3, W, H)
    rci = rtvk.RenderCallInfo.from_buffer_copy(rci_np.tobytes())
    ref_acc, ref_out, _ = oracle.render(bench.scene("canon"), rci_np, W, H, opts=oracle.options(rng_mode=rng_mode))

    def frame():
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        r.render_device(rci, acc, out, options=rtvk.make_options(rng_mode=rng_mode))
        torch.cuda.synchronize()
        return acc.cpu().numpy(), out.cpu().numpy()

    a0, o0 = frame()
    cost0 = r.tile_costs().copy()
    plan0 = r.launch_info()
    rays, ref_ids, ref_t = bench.family("canon", None, "generic")
    ids, t = bench.probe(rays[:5000], LBVH)
    assert_hits(LBVH, rays[:5000], ids, t, ref_ids[:5000], ref_t[:5000])
    assert r.launch_info()["chunks"] == 1
    np.testing.assert_array_equal(r.tile_costs(), cost0)
    a1, o1 = frame()
    assert r.launch_info()["form"] == plan0["form"]
    for a, o in ((a0, o0), (a1, o1)):
        np.testing.assert_array_equal(a, ref_acc)
        np.testing.assert_array_equal(o, ref_out)
    assert cost0.size == (W // 8) * (H // 8) and cost0.max() > 0
