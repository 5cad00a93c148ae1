"""The CPU oracle against every pin the reference offers and against the
committed golden fixtures (tests/golden/, made by tests/golden/make_golden.py)."""
import math
from pathlib import Path

import numpy as np
import pytest

import closest_hit_cases as ch
import scatter_cases as sc

GOLDEN = Path(__file__).resolve().parent / "golden"

# SURVEY.md §4 pin 1: random.glsl restated in C and Python during the survey.
RNG_KNOWN = [((0, 0), 0xC9A6502E, 0.317775071), ((1, 0), 0x469EAABE, 0.0754855275),
             ((0, 1), 0x641949FF, 0.102772832), ((959, 539), 0x84C2F065, 0.978126526),
             ((1919, 1079), 0xBB27E01B, 0.387065768)]


@pytest.mark.parametrize("xy,seed,first", RNG_KNOWN)
def test_rng_known_answers(oracle, xy, seed, first):
    s = oracle.pixel_seed(*xy, 0)
    assert s == seed
    assert oracle.random_floats(s, 1)[0] == pytest.approx(first, abs=5e-10)


def test_lcg_and_float_exact(oracle):
    # random.glsl:15-22: seed = 1664525 * seed + 1013904223; float(seed & 0xFFFFFF) / 2^24
    s = 0x12345678
    fl = oracle.random_floats(s, 4)
    for f in fl:
        s = (1664525 * s + 1013904223) & 0xFFFFFFFF
        assert f == (s & 0xFFFFFF) / 16777216.0


def _f(a, lo, hi):
    return a[lo:hi].copy().view(np.float32)


def test_scene_reference_pins(oracle):
    """SURVEY.md §4 pin 2 (from the reference's own scene.h compiled by g++ 11.4)."""
    sc = oracle.generate_scene(0.0)
    assert sc.shape == (488, 80)
    mat = sc[:, 16:20].copy().view(np.uint32).ravel()
    assert np.bincount(mat, minlength=3).tolist() == [360, 70, 58]
    np.testing.assert_array_equal(_f(sc[4], 0, 16), np.float32([-10.878071, 0.2, -10.266748, 0.2]))
    assert mat[4] == 2
    assert mat[6] == 0
    np.testing.assert_allclose(_f(sc[6], 32, 44), [0.168750, 0.450000, 0.112500], atol=1e-6)
    np.testing.assert_array_equal(_f(sc[487], 0, 16),
                                  np.float32([10.1279688, 0.200000003, 10.8928413, 0.200000003]))
    assert mat[487] == 0
    np.testing.assert_array_equal(_f(sc[487], 32, 48),
                                  np.float32([0.449999988, 0.163125008, 0.112500012, 1.0]))
    # fixed spheres, scene.h:85-116 at t = 0 (cos 0 = 1)
    np.testing.assert_array_equal(_f(sc[0], 0, 16), np.float32([0, -1000, 1, 1000]))
    for i, x in ((1, -4.0), (2, 4.0), (3, 0.0)):
        np.testing.assert_array_equal(_f(sc[i], 0, 16), np.float32([x, 1, 1, 1]))


def test_scene_time_dependence(oracle):
    t = 0.7
    sc = oracle.generate_scene(t)
    z = [float(_f(sc[i], 8, 12)[0]) for i in (1, 2, 3)]
    assert z == [np.float32(math.cos(2 * np.float32(t))), np.float32(math.cos(3 * np.float32(t))),
                 np.float32(math.cos(np.float32(t)))]
    np.testing.assert_array_equal(sc[4:], oracle.generate_scene(0.0)[4:])


def _fnv1a64(data: bytes, basis: int) -> int:
    h = basis
    for c in data:
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_scene_fnv_pin(oracle):
    """FNV-1a-64 over spheres[4..487] (the time-independent bytes, 38 720 B).

    SURVEY.md §4 quotes b1fa62b66a87952d, hashed from the reference's own src/scene.h compiled by
    g++ 11.4 during the survey. That hash used the offset basis 1469598103934665603 (the standard
    basis 14695981039346656037 with its last digit dropped). With that basis the oracle's scene
    reproduces the survey value exactly, so the scene is pinned byte for byte to the reference's
    generator. The standard-basis value of the same bytes is asserted too."""
    data = oracle.generate_scene(0.0)[4:].tobytes()
    assert len(data) == 484 * 80
    assert _fnv1a64(data, 1469598103934665603) == 0xB1FA62B66A87952D
    assert _fnv1a64(data, 14695981039346656037) == 0x9E1C4982E10FE953      # standard FNV basis


def test_big_grid_generator(oracle):
    sc = oracle.generate_scene(0.0, 158)
    assert sc.shape[0] == 4 + 316 * 316
    np.testing.assert_array_equal(sc[:4], oracle.generate_scene(0.0)[:4])


def test_sin_accuracy(oracle):
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-100, 100, 2000), rng.uniform(-6e4, 6e4, 2000),
                         np.arange(-50, 50) * np.pi]).astype(np.float32)
    for x in xs:
        got = oracle.sinf(float(x))
        ref = math.sin(float(x))
        assert abs(got - ref) <= 2e-7 + 2e-7 * abs(ref), (x, got, ref)


@pytest.mark.parametrize("case", ["g64x36_spp4", "g48x32_spp3_depth3_local", "g40x24_spp2_counter",
                                  "g56x40_spp7_hash"])
def test_golden_fixtures(oracle, case):
    import json
    meta = json.loads((GOLDEN / f"{case}.json").read_text())
    sc = oracle.generate_scene(meta["t"], meta["K"])
    rci = oracle.render_call_info(meta["spp"], meta["W"], meta["H"], tuple(meta["offset"]))
    op = oracle.options(max_depth=meta["max_depth"], seed_mode=meta["seed_mode"], rng_mode=meta["rng_mode"])
    acc, out, st = oracle.render(sc, rci, meta["band_w"], meta["band_h"], opts=op, threads=4)
    g = np.load(GOLDEN / f"{case}.npz", allow_pickle=False)
    np.testing.assert_array_equal(acc, g["accum"])
    np.testing.assert_array_equal(out, g["rgba8"])
    assert list(st) == g["stats"].tolist()


def test_band_split_invariance(oracle):
    """Global seeds make an image independent of how it is split into bands."""
    sc = oracle.generate_scene()
    W, H = 40, 30
    full_a, full_o, _ = oracle.render(sc, oracle.render_call_info(2, W, H), W, H, threads=4)
    top_a, top_o, _ = oracle.render(sc, oracle.render_call_info(2, W, H, (0, 0)), W, 11, threads=4)
    bot_a, bot_o, _ = oracle.render(sc, oracle.render_call_info(2, W, H, (0, 11)), W, 19, threads=4)
    np.testing.assert_array_equal(np.concatenate([top_a, bot_a]), full_a)
    np.testing.assert_array_equal(np.concatenate([top_o, bot_o]), full_o)
    rows = np.array([3, 17, 29, 0], np.uint32)  # strip tiling through the rows map
    r_a, r_o, _ = oracle.render(sc, oracle.render_call_info(2, W, H), W, 4, rows=rows, threads=2)
    np.testing.assert_array_equal(r_a, full_a[rows])


def test_launch_local_seed_mode(oracle):
    """shader.rgen:40 verbatim: the seed uses the band-local launch id."""
    sc = oracle.generate_scene()
    W, H = 24, 16
    full_a, _, _ = oracle.render(sc, oracle.render_call_info(1, W, H), W, H, opts=oracle.options(seed_mode=1))
    glob_a, _, _ = oracle.render(sc, oracle.render_call_info(1, W, H), W, H)
    np.testing.assert_array_equal(full_a, glob_a)   # offset 0: local == global
    bot_l, _, _ = oracle.render(sc, oracle.render_call_info(1, W, H, (0, 8)), W, 8, opts=oracle.options(seed_mode=1))
    assert not np.array_equal(bot_l, glob_a[8:])     # band-local seeds repeat the top band's stream


def test_counter_rng_sample_split(oracle):
    """RT_RNG_SAMPLE_COUNTER: 4 samples in one call == 2 + 2 (accumulate, sample_base)."""
    sc = oracle.generate_scene()
    W, H = 16, 12
    a4, _, _ = oracle.render(sc, oracle.render_call_info(4, W, H), W, H, opts=oracle.options(rng_mode=1))
    a2, _, _ = oracle.render(sc, oracle.render_call_info(2, W, H), W, H, opts=oracle.options(rng_mode=1))
    a22, _, _ = oracle.render(sc, oracle.render_call_info(2, W, H), W, H, accum=a2,
                              opts=oracle.options(rng_mode=1, accumulate=1, sample_base=2))
    # float accumulator rounding between the two calls: sums agree to float precision
    np.testing.assert_allclose(a22, a4, rtol=1e-6, atol=1e-6)


def test_empty_scene_is_sky(oracle):
    rci = oracle.render_call_info(3, 8, 4)
    acc, out, st = oracle.render(np.zeros((0, 80), np.uint8), rci, 8, 4)
    sky = np.float32([0.7, 0.8, 1.0]).astype(np.float64)
    expect = (sky + sky + sky).astype(np.float32)          # dvec3 sum, stored as float
    np.testing.assert_array_equal(acc[..., :3], np.broadcast_to(expect, (4, 8, 3)))
    px = np.sqrt(expect / np.float32(3)).astype(np.float32)
    assert out[0, 0].tolist() == [int(v * np.float32(255) + np.float32(0.5)) for v in px] + [255]
    assert st[0] == 3 * 32 and st[1] == 3 * 32


def test_depth_one_is_black_or_direct(oracle):
    """max_depth 1: a scattering first hit ends with light 0 (Q6); only absorbed hits or misses
    contribute (here: nothing misses, primaries all hit geometry)."""
    sc = oracle.generate_scene()
    acc, out, st = oracle.render(sc, oracle.render_call_info(2, 32, 18), 32, 18, opts=oracle.options(max_depth=1))
    assert st[0] == st[1]
    assert (acc[..., :3] == 0).mean() > 0.9


# ---- RT_RNG_SAMPLE_HASH --------------------------------------------------------
def _lowbias32(pixel_seed: int, s: int) -> int:
    """Python restatement of the sample-seed hash (golden-ratio spread + lowbias32 finaliser)."""
    m = 0xFFFFFFFF
    x = (pixel_seed + 0x9E3779B9 * s) & m
    x ^= x >> 16
    x = (x * 0x21F0AAAD) & m
    x ^= x >> 15
    x = (x * 0x735A2D97) & m
    x ^= x >> 15
    return x


def test_sample_seed_hash(oracle):
    rng = np.random.default_rng(7)
    for ps, s in [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xC9A6502E, 1)] + \
            [tuple(int(v) for v in rng.integers(0, 2**32, 2, dtype=np.uint64)) for _ in range(200)]:
        assert oracle.sample_seed_hash(ps, s) == _lowbias32(ps, s)
    # consecutive samples of one pixel start at well-spread LCG states
    seeds = [_lowbias32(0xC9A6502E, s) for s in range(4096)]
    assert len(set(seeds)) == 4096
    bits = np.unpackbits(np.array(seeds, np.uint32).view(np.uint8))
    assert abs(bits.mean() - 0.5) < 0.01


def test_sample_fixed(oracle):
    """trunc(clamp(c, 0, 1) * 2^24): exact for representable products, NaN -> 0."""
    rng = np.random.default_rng(3)
    cs = np.concatenate([rng.uniform(0, 1, 500), 10.0 ** rng.uniform(-40, 0, 500)]).astype(np.float32)
    for c in cs:
        assert oracle.sample_fixed(float(c)) == int(np.float32(c) * np.float32(2.0 ** 24))
    assert oracle.sample_fixed(1.0) == 2 ** 24
    assert oracle.sample_fixed(0.0) == 0 and oracle.sample_fixed(-0.5) == 0 and oracle.sample_fixed(3.0) == 2 ** 24
    assert oracle.sample_fixed(float("nan")) == 0
    assert oracle.sample_fixed(2.0 ** -25) == 0 and oracle.sample_fixed(2.0 ** -24) == 1


def test_hash_mode_frame(oracle):
    """RT_RNG_SAMPLE_HASH frames: the stored sum is float(double(fixed sum) * 2^-44); splitting the
    samples over two calls (accumulate + sample_base) agrees to float precision; the image is a
    different Monte-Carlo estimate of the same picture as the reference stream (mean within 2 %)."""
    sc = oracle.generate_scene()
    W, H, spp = 48, 27, 16
    hash_opts = oracle.options(rng_mode=2)
    a, o, st = oracle.render(sc, oracle.render_call_info(spp, W, H), W, H, opts=hash_opts)
    a8, _, _ = oracle.render(sc, oracle.render_call_info(8, W, H), W, H, opts=hash_opts)
    a88, _, _ = oracle.render(sc, oracle.render_call_info(8, W, H), W, H, accum=a8,
                              opts=oracle.options(rng_mode=2, accumulate=1, sample_base=8))
    np.testing.assert_allclose(a88[..., :3], a[..., :3], rtol=1e-6, atol=1e-6)
    assert (a[..., 3] == 1.0).all() and st[1] == W * H * spp
    ref, ro, _ = oracle.render(sc, oracle.render_call_info(spp, W, H), W, H)
    assert not np.array_equal(a, ref)
    assert abs(float(a[..., :3].mean()) / float(ref[..., :3].mean()) - 1.0) < 0.02
    # rgba8 is the tonemap of the stored sum, as for every mode
    np.testing.assert_array_equal(o, oracle.resolve(a, spp))


def test_sky_matches_reference_render(oracle):
    """The reference's own rendered output (/root/reference/sceneRender.png, via the fixture
    tests/golden/sceneRender_stats.npz made by tests/golden/make_scene_render_ref.py): its sky
    blocks (40x40-pixel means, top three rows, median) equal the oracle's sky pixel, i.e. the
    constant sky of shader.rmiss:15 through the tonemap of shader.rgen:65-66 and the UNORM store."""
    ref = np.load(GOLDEN / "sceneRender_stats.npz", allow_pickle=False)
    sky_ref = np.median(ref["thumb"][:3].reshape(-1, 3), axis=0)
    _, out, _ = oracle.render(np.zeros((0, 80), np.uint8), oracle.render_call_info(4, 8, 8), 8, 8)
    sky_ours = out[0, 0, :3].astype(np.float32)
    assert sky_ours.tolist() == [213.0, 228.0, 255.0]
    np.testing.assert_allclose(sky_ref, sky_ours, atol=0.5)


@pytest.mark.parametrize("rng,min_psnr", [(0, 35.0), (2, 45.0)])
def test_literal_glsl_forms_near_contract(oracle, rng, min_psnr):
    """The contract drift measure: the oracle's literal readings of the GLSL
    (LIT_RINT: shader.rint:33-55 as written, unfused D and / a; LIT_ALL: also every dot() and
    normalize() as written) against the shipped contract the kernels implement. They differ (in
    some pixels, through rounding-flipped branches) but stay close: at 96x54, 16 spp the image
    PSNR stays above the stated floor and the mean brightness within 1 %."""
    sc = oracle.generate_scene()
    rci = oracle.render_call_info(16, 96, 54)
    acc0, px0, st0 = oracle.render(sc, rci, 96, 54, opts=oracle.options(rng_mode=rng))
    for lit in (oracle.LIT_RINT, oracle.LIT_ALL):
        acc, px, st = oracle.render(sc, rci, 96, 54, opts=oracle.options(rng_mode=rng, lit=lit))
        assert not np.array_equal(acc, acc0)   # the forms really differ
        mse = np.mean((px[..., :3].astype(np.float64) - px0[..., :3]) ** 2)
        assert 10 * np.log10(255 ** 2 / mse) >= min_psnr
        assert abs(acc[..., :3].mean() / acc0[..., :3].mean() - 1) < 0.01
        assert abs(st[0] / st0[0] - 1) < 0.01


def test_literal_form_contract_unchanged(oracle):
    """Selecting the contract explicitly is the default render (the literal forms are opt-in)."""
    sc = oracle.generate_scene()
    rci = oracle.render_call_info(2, 40, 24)
    a0, p0, _ = oracle.render(sc, rci, 40, 24)
    a1, p1, _ = oracle.render(sc, rci, 40, 24, opts=oracle.options(lit=oracle.LIT_CONTRACT))
    assert np.array_equal(a0, a1) and np.array_equal(p0, p1)


# ---- the closest-hit checker (orc_closest_hits) against float64 and against orc_render --------

@pytest.fixture(scope="module")
def generic_f64(oracle):
    """Per scene: the generic family, the oracle's answers and float64's, computed once."""
    memo = {}

    def get(name):
        if name not in memo:
            sc = ch.make_scene(oracle, name)
            rays = ch.generic(ch.geometry(sc), ch.N_RAYS_BIG if name == "big" else ch.N_RAYS)
            memo[name] = (sc, rays, oracle.closest_hits(sc, rays), ch.closest_hits_f64(ch.geometry(sc), rays))
        return memo[name]
    return get


@pytest.mark.parametrize("scene", ch.SCENES + ("big",))
def test_closest_hits_agree_with_float64(oracle, generic_f64, scene):
    """Two restatements of one contract can share a mistake: the oracle's closest hit (binary32,
    the contract's operation order, gated) against the plain quadratic in float64 (closest t in
    [tmin, tmax], lowest index on ties) on the generic family. On the rays float64 can decide
    (closest_hit_cases.decided: the best two candidates apart, no discriminant near 0, no root near
    tmin or tmax) the winner is the same and t agrees within T_TOL_U * 2^-24 * tscale; at most 5 %
    of the family may be undecided."""
    sc, rays, (ids, t), (fi, ft, gap, disc, edge, tscale) = generic_f64(scene)
    dec = ch.decided(ft, gap, disc, edge)
    hit = dec & (fi != ch.MISS)
    ratio = np.abs(t[hit].astype(np.float64) - ft[hit]) / (2.0 ** -24 * tscale[hit])
    wrong = np.flatnonzero(ids != fi)
    print(f"{scene}: undecided {1 - dec.mean():.4f}, winners that differ {len(wrong)} (largest disc "
          f"{disc[wrong].max() if len(wrong) else 0:.3g}, smallest gap / max(1, t) "
          f"{(gap[wrong] / np.maximum(1, np.where(np.isfinite(ft[wrong]), ft[wrong], 1))).min() if len(wrong) else np.inf:.3g}, "
          f"smallest edge {edge[wrong].min() if len(wrong) else np.inf:.3g}), worst |t - t64| / (u tscale) "
          f"{ratio.max():.3g}")
    assert 1 - dec.mean() <= ch.UNDECIDED_MAX
    bad = np.flatnonzero(dec & (ids != fi))
    assert bad.size == 0, [(int(i), int(ids[i]), int(fi[i]), float(t[i]), float(ft[i])) for i in bad[:4]]
    assert ratio.max() <= ch.T_TOL_U
    assert (fi != ch.MISS).mean() > 0.5 and (fi == ch.MISS).mean() > 0.05   # the family hits and misses


@pytest.mark.parametrize("scene", ch.SCENES + ("big",))
def test_tangent_family_has_rounding_corners(oracle, scene):
    """The tangent family's condition on its own inputs: at least 32 rays whose ungated winner
    (the quadratic alone) fails the AABB gate, so that the contract's winner is another sphere or
    none. These are the rays on which a walk must notice that its winner is not the answer."""
    sc = ch.make_scene(oracle, scene)
    rays = ch.tangent(ch.geometry(sc), ch.N_RAYS_BIG if scene == "big" else ch.N_RAYS)
    gi, _ = oracle.closest_hits(sc, rays)
    ui, _ = oracle.closest_hits(sc, rays, gated=False)
    corners = int(((ui != gi) & (ui != ch.MISS)).sum())
    print(f"{scene}: {corners} corners of {len(rays)}")
    assert corners >= 32
    assert np.all((ui == gi) | (ui != ch.MISS))   # the gate only ever removes candidates


def test_closest_hits_match_render_hit_pattern(oracle):
    """orc_closest_hits against orc_render: a 1-spp, depth-1 frame ends at its camera ray's closest
    hit (a miss returns the sky colour, a hit black or the absorbing material's colour), so its
    hit-or-miss pattern is the probe's on the same camera rays (shader.rgen:56-58, 107-115 restated
    with numpy in binary32)."""
    W, H = 64, 36
    sc = oracle.generate_scene()
    rci = oracle.render_call_info(1, W, H)
    f = rci.view(np.float32)
    f[8:11] = [13.0, 1.0, 3.0]       # a low camera: the horizon crosses the frame
    f[12:15] = [-13.0, 0.5, -3.0]
    acc, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(max_depth=1))
    vp = np.zeros(18, np.float32)
    oracle.lib().orc_viewport(rci.ctypes.data, vp.ctypes.data)
    look_from, hor, ver, ulc = vp[0:3], vp[3:6], vp[6:9], vp[9:12]
    rays = np.zeros((H * W, 6), np.float32)
    for y in range(H):
        for x in range(W):
            r0, r1 = oracle.random_floats(oracle.pixel_seed(x, y), 2)
            ux = (np.float32(x) + np.float32(r0)) / np.float32(W)
            uy = (np.float32(y) + np.float32(r1)) / np.float32(H)
            to = (ulc + ux * hor) - uy * ver
            rays[y * W + x] = np.concatenate([look_from, to - look_from])
    ids, _ = oracle.closest_hits(sc, rays)
    sky = np.all(acc[..., :3] == np.float32([0.7, 0.8, 1.0]), axis=-1).reshape(-1)
    np.testing.assert_array_equal(sky, ids == ch.MISS)
    assert 0.1 < sky.mean() < 0.9


# ---- the shading checker (orc_scatter) against the float64 restatement of shader.rchit ----------

@pytest.fixture(scope="module")
def scatter_f64(oracle):
    """Per scene: every family's cases, the oracle's bounce and float64's, computed once."""
    memo = {}

    def get(name):
        if name not in memo:
            scene, fams = sc.all_cases(oracle, name)
            memo[name] = {fam: (args, oracle.scatter(scene, *args), sc.scatter_f64(scene, *args)) for fam, args in fams.items()}
        return memo[name]
    return get


def _assert_kept(what, args, orc, f64, keep):
    """The kept-case rules: does_scatter, the LCG state and the attenuation exactly, p and the raw
    scatter direction within their tolerances. Returns the worst p and sd ratios (the measured C)."""
    for name, ours, theirs in (("does_scatter", orc["scatter"].astype(bool), f64["scatter"]),
                               ("seed_after", orc["seed"], f64["seed"]),
                               ("attenuation", orc["att"].view(np.uint32), f64["att"].view(np.uint32))):
        diff = ours != theirs
        bad = np.flatnonzero(keep & (diff if diff.ndim == 1 else diff.any(axis=1)))
        assert bad.size == 0, (what, name, [(int(i), args[0][i].tolist(), int(args[1][i]), float(args[2][i]), int(args[3][i]))
                                            for i in bad[:3]])
    # d_next is normalize of the oracle's own sd (in float64: within 2 ulps per coordinate), zeros without a scatter
    sc_o = orc["scatter"].astype(bool)
    own = sc.normalize(np.where(sc_o[:, None], orc["sd"].astype(np.float64), 1.0))
    assert np.all(orc["d_next"][~sc_o] == 0.0)
    assert np.abs(orc["d_next"] - own)[keep & sc_o].max(initial=0.0) <= 4.0 * sc.U, what
    rp = np.abs(orc["p"] - f64["p"]).max(axis=1) / (sc.U * f64["p_scale"])
    rs = np.abs(orc["sd"] - f64["sd"]).max(axis=1) / (sc.U * f64["sd_scale"])
    cp, csd = (float(rp[keep].max()), float(rs[keep].max())) if keep.any() else (0.0, 0.0)
    assert cp <= sc.C_P and csd <= sc.C_SD, (what, cp, csd)
    return cp, csd


@pytest.mark.parametrize("family", [f for f in sc.FAMILIES if f != "head_on"])
@pytest.mark.parametrize("scene", sc.SCENES)
def test_scatter_agrees_with_float64(scatter_f64, scene, family):
    """closest_hit_shader and the kernels' shade_rec were written by the same hands from one reading
    of shader.rchit, and are only ever compared with each other: the oracle's bounce against a
    float64 restatement written from the GLSL. On the cases binary32 must decide as float64 does
    (scatter_cases.kept: every margin above tau = 1e-4, 1 - cos^2 above 2^-20, and a metal's margin
    above its resolution when reflect + fuzz ru is short) does_scatter, the LCG state afterwards and
    the attenuation are equal, d_next is normalize of the oracle's own sd, p lies
    within C_P 2^-24 (|o| + t) and the raw scatter direction within C_SD 2^-24 x its condition term;
    the share left out is at most 1 % (generic, bounce) or 60 % (the threshold families)."""
    args, orc, f64 = scatter_f64(scene)[family]
    keep = sc.kept(f64)
    excluded = 1.0 - keep.mean()
    cp, csd = _assert_kept(f"{scene} {family}", args, orc, f64, keep)
    by = {k: round(float(np.mean(v <= sc.TAU)), 4) for k, v in f64["margins"].items()}
    short_w = int(((f64["margins"]["metal"] > sc.TAU) & (f64["margins"]["metal"] <= f64["metal_resolution"])).sum())
    print(f"{scene} {family}: {len(keep)} cases, excluded {excluded:.4f} (below tau by margin {by}; {short_w} more cases by the "
          f"metal resolution), worst p ratio {cp:.2f}, worst sd ratio {csd:.2f}")
    assert excluded <= sc.EXCLUDED_MAX[family]
    assert keep.sum() >= 4096


@pytest.mark.parametrize("scene", sc.SCENES)
def test_scatter_head_on(oracle, scatter_f64, scene):
    """Rays aimed at a glass sphere's centre: cos_t = dot(-d, n) rounds above 1 in about one case of
    six, 1 - cos^2 is negative, its sqrt NaN, `eta * NaN <= 1` false: the bounce reflects without a
    draw, whatever the ior (1.0 included). That is shader.rchit:125-128 as written, so it is the
    contract. Every case in which the oracle takes no draw has a float64 1 - cos^2 below 2^-20; every
    other case obeys the kept-case rules."""
    args, orc, f64 = scatter_f64(scene)["head_on"]
    no_draw = orc["seed"] == args[3]
    assert np.all(f64["mtype"] == 2)
    assert np.all(f64["om"][no_draw] < sc.OM_MIN), float(f64["om"][no_draw].max())
    keep = sc.kept(f64, head_on=True) & ~no_draw
    cp, csd = _assert_kept(f"{scene} head_on", args, orc, f64, keep)
    R = sc.records(sc.make_scene(oracle, scene))
    share = {float(i): round(float(no_draw[R["attr"][args[1]] == np.float32(i)].mean()), 3) for i in sc.IORS}
    print(f"{scene} head_on: no-draw share per ior {share}; {int(keep.sum())} of {int((~no_draw).sum())} drawing cases kept, "
          f"worst p ratio {cp:.2f}, worst sd ratio {csd:.2f}")
    assert no_draw.sum() >= 256 and keep.sum() >= 4096
    # without a draw the bounce is the mirror's: straight back
    np.testing.assert_array_equal(orc["scatter"][no_draw], 1)
    d = sc.normalize(args[0][:, 3:].astype(np.float64))
    assert np.abs(orc["sd"][no_draw] + d[no_draw]).max() < 1e-5


def test_scatter_families_reach_their_edges(scatter_f64):
    """What the families are for, on their own inputs, in float64: back faces and rays inside glass
    (bounce), both sides of every threshold within TAU-decades of it (the threshold families), every
    material, every draw count, absorbed and scattered bounces."""
    for scene in sc.SCENES:
        fams = scatter_f64(scene)
        f = fams["generic"][2]
        assert set(np.unique(f["mtype"])) == {0, 1, 2, 3, 7} and set(np.unique(f["draws"])) == {0, 1, 3}
        assert (f["scatter"] == 0).sum() > 200
        f = fams["bounce"][2]
        back = ~f["front"] & (f["mtype"] <= 2)
        assert back.sum() > 500 and (back & (f["mtype"] == 2)).sum() > 100      # back faces; from inside glass
        args, _, f = fams["tir"]
        near = f["margins"]["can_refract"] < 1e-2
        assert (near & (f["draws"] == 0)).sum() > 2000 and (near & (f["draws"] == 1)).sum() > 2000
        f = fams["metal_edge"][2]
        near = f["margins"]["metal"] < 1e-2
        assert (near & f["scatter"]).sum() > 2000 and (near & ~f["scatter"]).sum() > 2000
        f = fams["diffuse_edge"][2]
        assert np.all(np.sqrt((f["sd"] ** 2).sum(axis=1)) < 0.05)       # |n + ru| with dot(ru, n) < -0.999
        f = fams["checker_edge"][2]
        assert (f["margins"]["checker"] < 1e-2).mean() > 0.7
        f = fams["grazing"][2]
        assert (f["margins"]["face"] < 1e-2).mean() > 0.7


def test_restatement_obeys_the_physics(oracle):
    """The float64 restatement is pinned to the laws it restates, at 1e-12, so that it is not one
    more private reading: the mirror law, Snell's law on the far side of the surface, unit length of
    a refracted unit vector, Schlick's end points, ior 1 refracting straight on, diffuse output on
    the normal's side, and the draw counts."""
    rng = np.random.default_rng(5)
    n = 4096
    unit = lambda: sc.normalize(rng.normal(size=(n, 3)))
    nrm, d = unit(), unit()
    d = np.where((sc.dot(d, nrm) > 0)[:, None], -d, d)          # incoming: against the normal
    # mirror law
    r = sc.reflect(d, nrm)
    assert np.abs(sc.dot(r, nrm) + sc.dot(d, nrm)).max() < 1e-12
    assert np.abs(np.cross(r - d, nrm)).max() < 1e-12
    # Snell, unit length, the far side
    for eta in (1.0 / 1.5, 1.0 / 1.33, 1.5, 2.4, 1.0 / 0.6):
        e = np.full(n, eta)
        sin_i = np.linalg.norm(np.cross(d, nrm), axis=1)
        ok = eta * sin_i < 1.0 - 1e-9
        tr = sc.refract(d, nrm, e)
        assert ok.sum() > 100
        assert np.abs(np.linalg.norm(np.cross(tr, nrm), axis=1) - eta * sin_i)[ok].max() < 1e-12
        assert np.abs(np.linalg.norm(tr, axis=1) - 1.0)[ok].max() < 1e-12
        assert np.all(sc.dot(tr, nrm)[ok] < 0.0)
        assert np.abs(np.cross(np.cross(d, nrm), np.cross(tr, nrm))).max() < 1e-12   # in the plane of incidence
        assert np.all(tr[eta * sin_i > 1.0 + 1e-9] == 0.0)     # beyond the critical angle: GLSL's zero vector
    assert np.abs(sc.refract(d, nrm, np.ones(n)) - d).max() < 1e-12
    # Schlick
    for eta in (0.6, 1.0 / 1.5, 1.0, 1.5, 2.4):
        e = np.full(3, eta)
        s = sc.schlick(np.array([1.0, 0.0, 0.5]), e)
        r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
        assert abs(s[0] - r0) < 1e-12 and abs(s[1] - 1.0) < 1e-12 and r0 <= s[2] <= 1.0
    # the whole bounce on a hand-made scene: one sphere of each material at the origin
    base = oracle.generate_scene()[4:5]
    for mtype, attr, draws in ((0, 0.0, 3), (1, 0.3, 3), (2, 1.5, 1), (2, 1.0, 1), (3, 0.0, 0), (7, 0.5, 0)):
        rec = base.copy()
        rec[0, :16].view(np.float32)[:] = [0.0, 0.0, 0.0, 1.0]
        sc._write(rec[0], mtype, 0, (0.5, 0.6, 0.7), (0.1, 0.2, 0.3), attr)
        o = (unit() * 3.0).astype(np.float32)
        tgt = unit() * 0.7
        rays = np.concatenate([o, (tgt - o).astype(np.float32)], axis=1).astype(np.float32)
        dd = sc.normalize(rays[:, 3:].astype(np.float64))
        b = sc.dot(o.astype(np.float64), dd)
        t = (-b - np.sqrt(b * b - (sc.dot(o.astype(np.float64), o.astype(np.float64)) - 1.0))).astype(np.float32)
        f = sc.scatter_f64(rec, rays, np.zeros(n, np.uint32), t, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        assert np.all(f["draws"] == draws), (mtype, attr)
        nn = sc.normalize(f["p"])
        if mtype == 0:
            assert np.all(sc.dot(f["sd"], nn) >= 0.0)
        if mtype >= 3:
            assert not f["scatter"].any()
        if mtype == 2 and attr == 1.0:
            refr = np.abs(f["sd"] - dd).max(axis=1) < 1e-12
            assert refr.mean() > 0.9 and np.abs(f["sd"][~refr] - sc.reflect(dd, nn)[~refr]).max() < 1e-12
    # total internal reflection: inside glass beyond the critical angle there is no draw
    rec = base.copy()
    rec[0, :16].view(np.float32)[:] = [0.0, 0.0, 0.0, 1.0]
    sc._write(rec[0], 2, 0, (1, 1, 1), (0, 0, 0), 1.5)
    o = np.float32([[0.9, 0.0, 0.0]])
    f = sc.scatter_f64(rec, np.concatenate([o, np.float32([[0.0, 1.0, 0.0]])], axis=1), np.zeros(1, np.uint32),
                       np.float32([np.sqrt(1 - 0.81)]), np.uint32([7]))
    assert f["draws"][0] == 0 and f["seed"][0] == 7 and f["scatter"][0]      # sin = 0.9 > 1 / 1.5
