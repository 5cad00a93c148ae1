"""The geometry contract through every walk: degenerate spheres against the oracle.

Finite geometry of any sign or size is rendered exactly as the CPU oracle renders it: negative and
zero radii, exact duplicates (the lowest index wins a tie in t), concentric shells, segments that
start inside a sphere, spheres that straddle tMax, radii at the scale of tMin and radius ratios
beyond what the host grid accepts. A sphere with a NaN or infinite centre or radius is refused with
RT_ERR_INVALID_ARGUMENT before any builder or trace kernel sees it, and the context keeps its scene.

Every case renders one 48 x 32 frame at 2 spp per variant and compares every accumulator float, every
rgba8 byte and the (segments, samples) counts with the oracle, in the brute-force, tree and grid
forms, both random streams, host and device builds. Each case first shows from the oracle alone
that it is not vacuous: the edge spheres E change at least 5 % of the frame's pixels (the measured
shares stand in the docstrings; they depend on the oracle only, not on the code under test).
The kernel form that ran is asserted through launch_info(): a grid form the scene cannot have
falls back to a tree walk, it is never skipped.
"""
import numpy as np
import pytest

from test_gpu_parity import (BRUTE, GRID, GRID_COOP, GRID_CQ, HASH, LBVH, LBVH_GLOBAL, LBVH_OCT, STREAM, WALK_FORM,
                             assert_same, tree_builder)

pytestmark = pytest.mark.gpu
FORMS = (BRUTE, LBVH, LBVH_OCT, LBVH_GLOBAL, GRID, GRID_COOP, GRID_CQ)
GRID_FORMS = (GRID, GRID_COOP, GRID_CQ)
W, H, SPP = 48, 32, 2
DIFFUSE, METAL, GLASS = 0, 1, 2


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
def renderer(rtvk):
    r = rtvk.Renderer(0)
    yield r
    r.close()


# ---- scenes and cameras (CPU only) ---------------------------------------------------------------
def geometry(sc):
    """(n, 4) float32 copy of the records' centre.xyz, radius."""
    return np.ascontiguousarray(sc[:, :16]).view(np.float32).reshape(-1, 4).copy()


def with_geometry(sc, g):
    out = np.ascontiguousarray(sc).copy()
    out[:, :16] = np.ascontiguousarray(g, np.float32).view(np.uint8).reshape(-1, 16)
    return out


def sphere(c, r, material=DIFFUSE, colour=(0.5, 0.5, 0.5), attr=0.0, colour1=None):
    """One 80-byte record (include/rt_abi.h Sphere)."""
    rec = np.zeros((1, 80), np.uint8)
    rec[0, :16] = np.array([c[0], c[1], c[2], r], np.float32).view(np.uint8)
    rec[0, 16:24] = np.array([material, 0 if colour1 is None else 1], np.uint32).view(np.uint8)
    rec[0, 32:48] = np.array([*colour, 0.0], np.float32).view(np.uint8)
    rec[0, 48:64] = np.array([*(colour1 or (0.0, 0.0, 0.0)), 0.0], np.float32).view(np.uint8)
    rec[0, 64:68] = np.array([attr], np.float32).view(np.uint8)
    return rec


def camera(oracle, cam, at, image=(W, H), offset=(0, 0), spp=SPP):
    """RenderCallInfo looking from cam at `at`; image / offset: the W x H band is a window of a
    larger image (the field of view is fixed at 25 degrees over the image: a window narrows it)."""
    rci = oracle.render_call_info(spp, image[0], image[1], offset)
    f = rci.view(np.float32)
    f[8:11] = cam
    f[12:15] = [at[k] - cam[k] for k in range(3)]
    return rci


def share(o1, o2):
    """Share of the frame's pixels whose rgba8 differs."""
    return float((o1 != o2).any(axis=-1).mean())


_REF = {}


def reference(oracle, key, sc, rci, rng):
    """The oracle's frame (accum, rgba8, stats), computed once per (case, variant, stream)."""
    k = (key, rng)
    if k not in _REF:
        _REF[k] = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=rng))
    return _REF[k]


def ground(oracle):
    return oracle.generate_scene()[:1].copy()


# ---- GPU side ------------------------------------------------------------------------------------
def render_current(rtvk, renderer, torch, rci_u32, accel, rng):
    """One frame of the renderer's current scene in kernel form `accel`."""
    rci = rtvk.RenderCallInfo.from_buffer_copy(np.ascontiguousarray(rci_u32).tobytes())
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda")
    opt = rtvk.make_options(rng_mode=rng, accel=LBVH if accel in WALK_FORM else accel)
    opt.reserved[1] = WALK_FORM.get(accel, 0)
    renderer.render_device(rci, acc, out, options=opt)
    torch.cuda.synchronize()
    st = renderer.stats()
    return acc.cpu().numpy(), out.cpu().numpy(), (st.segments, st.samples)


def check_forms(rtvk, renderer, torch, oracle, key, sc, rci, grid, forms=FORMS):
    """The renderer's current scene (== sc) equals the oracle in every form, both streams. grid:
    whether the scene has a uniform grid for this camera; without one a grid form runs a tree walk."""
    for rng in (STREAM, HASH):
        ra, ro, rst = reference(oracle, key, sc, rci, rng)
        for accel in forms:
            a, o, st = render_current(rtvk, renderer, torch, rci, accel, rng)
            form = renderer.launch_info()["form"]
            if accel == BRUTE:
                assert form == "brute", form
            elif accel in GRID_FORMS:
                assert form.startswith("grid" if grid else "lbvh"), (accel, form)
            elif accel in (LBVH_OCT, LBVH_GLOBAL):
                assert form.startswith("lbvh"), (accel, form)
            else:
                assert form != "brute", form
            assert_same(a, o, ra, ro)
            assert st == rst[:2], (accel, rng, st, rst)


def set_scene(renderer, sc, builder):
    with tree_builder(builder):
        renderer.set_scene(np.ascontiguousarray(sc, np.uint8).reshape(-1, 80))
    return renderer.scene_array(8)


# ---- negative radii ------------------------------------------------------------------------------
NEG_CAM = ((4.5, 1.6, -4.5), (0.0, 0.2, 0.0))


def negative_scenes(oracle):
    """{variant: (scene, scene without E, all-positive twin)} of the canonical K = 3 scene."""
    sc = oracle.generate_scene(0.0, 3)
    g = geometry(sc)
    third = np.arange(len(g)) >= 4
    third &= (np.arange(len(g)) % 3 == 0)
    gs = g.copy()
    gs[third, 3] *= -1.0
    gg = g.copy()
    gg[0, 3] = -1000.0
    return {"small": (with_geometry(sc, gs), sc[~third], sc),
            "ground": (with_geometry(sc, gg), sc[1:], sc)}


@pytest.mark.parametrize("builder", [None, "gpu"])
@pytest.mark.parametrize("variant", ["small", "ground"])
def test_negative_radii(rtvk, renderer, torch, oracle, variant, builder):
    """A sphere of radius -r renders exactly as one of radius r (the oracle's r * r, its fmin / fmax
    slab test and normalize(p - c) are blind to the sign): every third small sphere of the canonical
    K = 3 scene negated, and the ground sphere negated to -1000. The builders size boxes, cells, the
    big-sphere selection and the cull slacks by |r|: n_big and small_rmax equal the all-positive
    scene's. Not vacuous: removing the negated spheres changes 11.3 % (small) and 75.1 % (ground) of the
    oracle's pixels; the frame equals the all-positive scene's frame."""
    sc, without, positive = negative_scenes(oracle)[variant]
    rci = camera(oracle, *NEG_CAM)
    ref = reference(oracle, ("neg", variant), sc, rci, STREAM)
    assert share(ref[1], reference(oracle, ("neg-without", variant), without, rci, STREAM)[1]) >= 0.05
    np.testing.assert_array_equal(ref[0], reference(oracle, "neg-positive", positive, rci, STREAM)[0])
    want = set_scene(renderer, positive, builder)
    info = set_scene(renderer, sc, builder)
    assert (info["n_big"], info["small_rmax"]) == (want["n_big"], want["small_rmax"]) == (4, pytest.approx(0.2))
    check_forms(rtvk, renderer, torch, oracle, ("neg", variant), sc, rci, grid=True)


# ---- duplicates ----------------------------------------------------------------------------------
DUP_CAM = ((0.0, 4.0, -9.0), (0.0, 0.3, 0.0))
DUP_MATERIALS = [(DIFFUSE, (0.9, 0.1, 0.1), 0.0, None), (METAL, (0.1, 0.9, 0.1), 0.05, None),
                 (GLASS, (0.2, 0.2, 1.0), 1.5, None), (DIFFUSE, (1.0, 1.0, 0.0), 0.0, (0.0, 1.0, 1.0))]


DUP_COLOURS = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.2, 0.2, 1.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0),
               (1.0, 0.5, 0.0), (0.6, 0.6, 0.6), (0.1, 0.1, 0.1)]


def duplicate_scenes(oracle):
    """20 positions x 9 identical spheres (same centre, same radius) cycling diffuse, metal,
    dielectric and checkered materials, each of the nine its own colour (the first and the last of
    a position share the material, 8 = 0 mod 4, never the colour), and the same records in
    reversed order."""
    recs = []
    for p in range(20):
        c = (-3.6 + 1.8 * (p % 5), 0.6, -2.4 + 1.6 * (p // 5))
        for k in range(9):
            m, _, attr, col1 = DUP_MATERIALS[(p + k) % 4]
            recs.append(sphere(c, 0.6, m, DUP_COLOURS[k], attr, col1))
    dups = np.concatenate(recs)
    return {"forward": np.concatenate([ground(oracle), dups]),
            "reversed": np.concatenate([ground(oracle), dups[::-1]])}


@pytest.mark.parametrize("builder", [None, "gpu"])
def test_duplicates_lowest_index_wins(rtvk, renderer, torch, oracle, builder):
    """Nine identical spheres at each of 20 positions (more than one leaf's worth, every cell's list
    full of exact ties in t) of four materials: the lowest index wins every tie, as in the oracle's
    in-order `t < best`. The records in reversed order give another image (the oracle's two frames
    differ in 56.0 % of the pixels), and each order equals its own oracle frame in every walk."""
    scenes = duplicate_scenes(oracle)
    rci = camera(oracle, *DUP_CAM)
    fwd = reference(oracle, ("dup", "forward"), scenes["forward"], rci, STREAM)
    rev = reference(oracle, ("dup", "reversed"), scenes["reversed"], rci, STREAM)
    assert share(fwd[1], rev[1]) >= 0.05
    for variant, sc in scenes.items():
        set_scene(renderer, sc, builder)
        check_forms(rtvk, renderer, torch, oracle, ("dup", variant), sc, rci, grid=True)


# ---- concentric shells, camera inside ------------------------------------------------------------
def inside_scenes(oracle):
    """{variant: (scene, scene without E, camera, look-at)}."""
    base = oracle.generate_scene(0.0, 3)
    out = {}
    for name, r_in in (("shell_pos", 0.9), ("shell_neg", -0.9)):
        # radius 1.0 / 0.9 (above twice the median radius: tested exhaustively) and the same shell at
        # 0.4 / 0.36 (in the tree and the grid)
        shell = np.concatenate([sphere((3.0, 1.0, -3.0), 1.0, GLASS, (1.0, 1.0, 1.0), 1.5),
                                sphere((4.2, 0.4, -1.6), 0.4, GLASS, (1.0, 1.0, 1.0), 1.5),
                                sphere((3.0, 1.0, -3.0), r_in, GLASS, (1.0, 1.0, 1.0), 1.5),
                                sphere((4.2, 0.4, -1.6), 0.4 * r_in, GLASS, (1.0, 1.0, 1.0), 1.5)])
        out[name] = (np.concatenate([base, shell]), np.concatenate([base, shell[:2]]),
                     (7.0, 2.0, -6.0), (3.4, 0.8, -2.6))
    for name, mat, colour, attr in (("in_diffuse", DIFFUSE, (0.8, 0.6, 0.4), 0.0), ("in_glass", GLASS, (1.0, 1.0, 1.0), 1.5)):
        for tag, cam in (("", (5.5, 1.5, -4.3)), ("_axis", (5.0, 1.5, 0.0))):   # nonzero / one zero component
            centre = (cam[0] - 0.5, cam[1] + 0.25, cam[2] + 0.7)
            big = sphere(centre, 3.0, mat, colour, attr)
            out[name + tag] = (np.concatenate([base, big]), base, cam, (0.0, 0.5, 0.0))
    return out


@pytest.mark.parametrize("builder", [None, "gpu"])
@pytest.mark.parametrize("variant", ["shell_pos", "shell_neg", "in_diffuse", "in_diffuse_axis", "in_glass",
                                     "in_glass_axis"])
def test_concentric_and_camera_inside(rtvk, renderer, torch, oracle, variant, builder):
    """A glass shell (radius 1.0 around a concentric 0.9, once +0.9 and once -0.9) and a camera
    inside a radius-3 diffuse sphere and inside a radius-3 dielectric: segments that start inside a
    sphere take the far root (t1 < tMin selects t2). The shell stands twice: at radius 1.0 (above
    twice the median radius, so in the exhaustive list) and at 0.4 (in the tree and the grid). Cameras with every component nonzero (the
    kernels start camera rays at the camera position itself, pinhole_origin) and with a zero
    component (the general form). Not vacuous: without the inner sphere / the enclosing sphere the
    oracle's frame differs in 42.4 % (shells), 100 % (diffuse) and 73.0 % / 54.0 % (glass) of the pixels."""
    sc, without, cam, at = inside_scenes(oracle)[variant]
    rci = camera(oracle, cam, at)
    ref = reference(oracle, ("inside", variant), sc, rci, STREAM)
    assert share(ref[1], reference(oracle, ("inside-without", variant), without, rci, STREAM)[1]) >= 0.05
    set_scene(renderer, sc, builder)
    check_forms(rtvk, renderer, torch, oracle, ("inside", variant), sc, rci, grid=True)
    assert renderer.launch_info()["pinhole_origin"] == (not variant.endswith("_axis"))


# ---- tMax ----------------------------------------------------------------------------------------
TMAX_IMAGE, TMAX_OFFSET = (336, 224), ((336 - W) // 2, (224 - H) // 2)


def tmax_scene(oracle, far_camera):
    """A 12 x 8 array of radius-40 spheres about 10 000 units from the camera, 80 apart, on a shell
    around the camera whose radius grows from 9 990 (left column) to 10 070 (right column): the
    nearest points of the spheres lie at t = 9 950-10 030 around tMax = 10 000, and the spheres in
    between are cut by it. The 48 x 32 band is the central window of a 336 x 224 image (the field of
    view is fixed: 20 units per pixel at that distance).
    far_camera: the array around the origin and the camera 10 000 away (beyond the padded radius:
    the tree is re-padded, the grid's margin does not cover the camera); else the camera near the
    origin and the array 10 000 away."""
    recs = []
    eye = np.array([0.0, 0.0, -10000.0]) if far_camera else np.array([0.5, 0.25, -3.0])
    for j in range(8):
        for i in range(12):
            m, col, attr, col1 = DUP_MATERIALS[(i + j) % 2 * 3]   # diffuse red / checkered yellow-cyan
            to = np.array([80.0 * (i - 5.5), 80.0 * (j - 3.5), 10000.0])
            c = eye + to / np.linalg.norm(to) * (10030.0 + (i - 5.5) / 5.5 * 40.0)
            recs.append(sphere(c, 40.0, m, col, attr, col1))
    return np.concatenate(recs), tuple(eye), tuple(eye + [0.0, 0.0, 10000.0])


@pytest.mark.parametrize("builder", [None, "gpu"])
@pytest.mark.parametrize("far_camera", [True, False])
def test_tmax_straddle(rtvk, renderer, torch, oracle, far_camera, builder):
    """Spheres straddling tMax = 10 000: a report at exactly tMax is accepted, one past it is not,
    in every walk (the walks start from best = 10 000 and compare packed keys). Not vacuous, from
    the oracle alone: rendered one at a time, 56 of the 96 spheres show (accepted, most of them cut)
    and 40 leave the all-sky frame untouched (rejected), and the whole frame differs from the
    all-sky frame in 42.5 % of the pixels (far camera and far array alike). The far camera re-pads the
    tree: the unpadded node copy, scene_array(5), is untouched."""
    sc, cam, at = tmax_scene(oracle, far_camera)
    rci = camera(oracle, cam, at, TMAX_IMAGE, TMAX_OFFSET)
    ref = reference(oracle, ("tmax", far_camera), sc, rci, STREAM)
    sky = reference(oracle, ("tmax-sky", far_camera), sc[:0], rci, STREAM)
    shown = [share(reference(oracle, ("tmax-one", far_camera, k), sc[k:k + 1], rci, STREAM)[1], sky[1]) > 0.0
             for k in range(len(sc))]
    assert min(sum(shown), len(shown) - sum(shown)) >= 24, sum(shown)
    assert 0.2 <= share(ref[1], sky[1]) <= 0.8
    set_scene(renderer, sc, builder)
    raw = renderer.scene_array(5).copy()
    # far camera: outside the grid's margin, a grid form walks the tree; far array: the grid runs
    check_forms(rtvk, renderer, torch, oracle, ("tmax", far_camera), sc, rci, grid=not far_camera)
    np.testing.assert_array_equal(raw, renderer.scene_array(5))


# ---- zero radii and radii at the scale of tMin ------------------------------------------------------
TINY_AT = (6.0, 2.0)                       # x, z of the patch of tiny spheres on the ground
TINY_IMAGE = (4800, 3200)                  # the band is its central window: 0.36 mm per pixel at 2.6 units
TINY_OFFSET = ((4800 - W) // 2, (3200 - H) // 2)
TINY_Y = float(np.sqrt(1e6 - TINY_AT[0] ** 2 - TINY_AT[1] ** 2) - 1000.0)   # the ground sphere's top there
TINY_CAM = ((TINY_AT[0] + 1.5, 1.5, TINY_AT[1] - 1.5), (TINY_AT[0], TINY_Y, TINY_AT[1]))


def tiny_scenes(oracle):
    """The canonical K = 3 scene plus 200 spheres of radius 0 and 200 of radius 0.0005-0.002 resting
    on the ground in a 16 x 10 mm patch, interleaved. Returns (scene, scene without the tiny ones)."""
    rng = np.random.default_rng(5)
    base = oracle.generate_scene(0.0, 3)
    mats = oracle.generate_scene(0.0, 11)[4:]
    recs, tiny = [], []
    for k in range(400):
        r = 0.0 if k % 2 == 0 else float(rng.uniform(0.0005, 0.002))
        x = TINY_AT[0] + float(rng.uniform(-0.008, 0.008))
        z = TINY_AT[1] + float(rng.uniform(-0.005, 0.005))
        y = float(np.sqrt(1e6 - x * x - z * z) - 1000.0) + r
        rec = mats[k % len(mats)].copy()[None]
        rec[0, :16] = np.array([x, y, z, r], np.float32).view(np.uint8)
        recs.append(rec)
        tiny.append(r > 0.0)
    extra = np.concatenate(recs)
    return np.concatenate([base, extra]), np.concatenate([base, extra[~np.array(tiny)]])


@pytest.mark.parametrize("builder", [None, "gpu"])
def test_zero_and_tmin_scale_radii(rtvk, renderer, torch, oracle, builder):
    """Zero-radius records among real spheres (the kernels' own padding relies on "radius 0 never
    reports") and radii of 0.0005-0.002, the scale of tMin = 0.001, seen from 2.6 units through a
    narrow window. The host grid refuses the scene (radii beyond 8 : 1) and a tree walk runs in its
    place; the device grid has no such limit (its reference bound holds) and runs. Not vacuous:
    without the 200 tiny spheres the oracle's frame differs in 69.1 % of the pixels."""
    sc, without = tiny_scenes(oracle)
    rci = camera(oracle, *TINY_CAM, TINY_IMAGE, TINY_OFFSET)
    ref = reference(oracle, "tiny", sc, rci, STREAM)
    assert share(ref[1], reference(oracle, "tiny-without", without, rci, STREAM)[1]) >= 0.05
    set_scene(renderer, sc, builder)
    check_forms(rtvk, renderer, torch, oracle, "tiny", sc, rci, grid=builder == "gpu")


# ---- radius ratio beyond the grid's ----------------------------------------------------------------
RATIO_CAM = ((13.0, 5.0, -6.0), (0.0, 0.5, 0.0))


def ratio_scenes(oracle):
    """The canonical scene plus 40 spheres of radius 0.01 and 70 of radius 1.9 on two rings: with
    the ground that is 74 spheres above twice the median radius, so the 64 largest are tested
    exhaustively and seven of radius 1.9 and the three of radius 1 fall into the tree beside radii
    0.2 and 0.01 (190 : 1). Returns (scene, canonical scene)."""
    rng = np.random.default_rng(9)
    base = oracle.generate_scene(0.0, 11)
    mats = base[4:]
    recs = []
    for k in range(40):
        x, z = float(rng.uniform(-3, 9)), float(rng.uniform(-6, 3))
        rec = mats[k].copy()[None]
        rec[0, :16] = np.array([x, 0.01 + float(np.sqrt(1e6 - x * x - z * z) - 1000.0), z, 0.01], np.float32).view(np.uint8)
        recs.append(rec)
    for k in range(70):
        ring, a = (9.0, 2 * np.pi * k / 35) if k < 35 else (15.0, 2 * np.pi * (k + 0.5) / 35)
        rec = mats[40 + k].copy()[None]
        rec[0, :16] = np.array([ring * np.cos(a), 1.9, ring * np.sin(a), 1.9], np.float32).view(np.uint8)
        recs.append(rec)
    return np.concatenate([base] + recs), base


@pytest.mark.parametrize("builder", [None, "gpu"])
def test_radius_ratio_beyond_grid(rtvk, renderer, torch, oracle, builder):
    """Radii of 0.01 and 1.9 mixed into the canonical scene, which alone takes the grid: more big
    spheres than the exhaustive list holds (64 of 74), the rest in the tree at a 190 : 1 ratio. The
    host grid refuses (8 : 1) and its forms walk the tree; the device grid, bounded by its reference
    count alone, runs. The image is exact whichever form the policy picks. Not vacuous: the added
    spheres change 97.9 % of the oracle's pixels."""
    sc, base = ratio_scenes(oracle)
    rci = camera(oracle, *RATIO_CAM)
    ref = reference(oracle, "ratio", sc, rci, STREAM)
    assert share(ref[1], reference(oracle, "ratio-base", base, rci, STREAM)[1]) >= 0.05
    info = set_scene(renderer, sc, builder)
    assert info["n_big"] == 64 and info["small_rmax"] == pytest.approx(1.9)
    check_forms(rtvk, renderer, torch, oracle, "ratio", sc, rci, grid=builder == "gpu")


# ---- refit ---------------------------------------------------------------------------------------
REFIT_CAM = ((4.5, 1.6, -4.5), (0.0, 0.2, 0.0))


def refit_scenes(oracle):
    """(K = 11 scene, its degenerate copy): of the small spheres, every fifth zeroed, every fifth
    negated and every fifth given the geometry of the sphere before it (an exact duplicate)."""
    sc = oracle.generate_scene(0.0, 11)
    g = geometry(sc)
    i = np.arange(len(g))
    small = i >= 4
    g[small & (i % 5 == 0), 3] = 0.0
    g[small & (i % 5 == 1), 3] *= -1.0
    dup = np.flatnonzero(small & (i % 5 == 3))
    g[dup] = g[dup - 1]
    return sc, with_geometry(sc, g)


def test_refit_into_degenerate(rtvk, renderer, torch, oracle):
    """A device-built K = 11 scene refitted (same topology) to a copy whose small spheres are partly
    zeroed, negated and duplicated: boxes, cells and radius bounds follow |r|, the image equals the
    oracle's in every form. Not vacuous: the oracle's frames of the two scenes differ in 24.0 % of
    the pixels."""
    sc, degenerate = refit_scenes(oracle)
    rci = camera(oracle, *REFIT_CAM)
    ref = reference(oracle, "refit", degenerate, rci, STREAM)
    assert share(ref[1], reference(oracle, "refit-before", sc, rci, STREAM)[1]) >= 0.05
    set_scene(renderer, sc, "gpu")
    nodes = renderer.scene_array(4).view(np.uint32).reshape(-1, 8)[:, [3, 7]].copy()
    with tree_builder("gpu"):
        renderer.refit_scene(degenerate)
    info = renderer.scene_array(8)
    assert info["device_built"] and info["small_rmax"] == pytest.approx(0.2)
    np.testing.assert_array_equal(nodes, renderer.scene_array(4).view(np.uint32).reshape(-1, 8)[:, [3, 7]])   # a refit
    check_forms(rtvk, renderer, torch, oracle, "refit", degenerate, rci, grid=True)


# ---- non-finite geometry -------------------------------------------------------------------------
def poisoned(sc, index, column, value):
    g = geometry(sc)
    g[index, column] = value
    return with_geometry(sc, g)


def assert_refused(rtvk, call, index):
    with pytest.raises(rtvk.RtError) as e:
        call()
    assert e.value.code == -1, e.value
    assert f"sphere {index}:" in str(e.value), e.value


def test_nonfinite_refused(rtvk, renderer, torch, oracle):
    """A sphere with a NaN or infinite centre or radius is refused with RT_ERR_INVALID_ARGUMENT (-1)
    and a message naming the first such sphere: host spheres before any builder runs (set_scene with
    the host and the device builder, refit_scene), device-resident spheres by the device build's
    own pass over them, before the grid build. No trace kernel is launched on a refused scene: the
    context keeps the scene it had, which renders bit-exactly after every refusal."""
    sc = oracle.generate_scene(0.0, 11)
    n = len(sc)
    rci = camera(oracle, *REFIT_CAM)
    bad = [(poisoned(sc, 0, 3, np.nan), 0), (poisoned(sc, n - 1, 0, np.inf), n - 1),
           (poisoned(sc, n // 2, 3, -np.inf), n // 2),
           (poisoned(poisoned(sc, 7, 1, np.nan), 300, 3, np.nan), 7)]
    for builder in (None, "gpu"):
        set_scene(renderer, sc, builder)
        for spheres, index in bad:
            with tree_builder(builder):
                assert_refused(rtvk, lambda: renderer.set_scene(spheres), index)
                assert_refused(rtvk, lambda: renderer.refit_scene(spheres), index)
        check_forms(rtvk, renderer, torch, oracle, "refused-keeps", sc, rci, grid=True, forms=(LBVH, GRID, LBVH_GLOBAL))
    # device-resident spheres: two 5-sphere scenes, each refused once; the K = 11 scene stays
    five = sc[:5]
    for spheres, index in ((poisoned(five, 3, 3, np.nan), 3), (poisoned(five, 1, 2, np.inf), 1)):
        dev = torch.from_numpy(spheres).cuda()
        assert_refused(rtvk, lambda: renderer.set_scene_device(dev), index)
    assert renderer.scene_array(8)["n_spheres"] == n
    check_forms(rtvk, renderer, torch, oracle, "refused-keeps", sc, rci, grid=True, forms=(LBVH, GRID, BRUTE))
    # ... and a refit of it still works (a full build: the refused build overwrote the topology)
    with tree_builder("gpu"):
        renderer.refit_scene(sc)
    check_forms(rtvk, renderer, torch, oracle, "refused-keeps", sc, rci, grid=True, forms=(LBVH,))
    # rt_multi (two logical devices): refused before the stored scene or any device's is touched
    ra, ro, _ = reference(oracle, "refused-keeps", sc, rci, STREAM)
    with rtvk.MultiRenderer(2, logical=True) as m:
        m.set_scene(sc)
        for spheres, index in bad:
            assert_refused(rtvk, lambda: m.set_scene(spheres), index)
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        m.render(rtvk.RenderCallInfo.from_buffer_copy(rci.tobytes()), acc, out)
        torch.cuda.synchronize()
        assert_same(acc.cpu().numpy(), out.cpu().numpy(), ra, ro)
