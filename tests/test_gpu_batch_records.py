"""The camera-batch form's records on the GPU (csrc/rt_trace_batch.h): a queue entry
holds no thr (a popped path's thr is rebuilt from the material record 2 bi + alt its word names), the
winner's gate record {c, r} comes from the block's LDS table by sphere id, and a generation batch
takes its camera-origin terms (oc and c of the first four big spheres, the grid's entry box from
cam.lf) from a table staged once per block.

Every case renders the same launch twice, with the form (the default) and with the unit loop
(rt_debug_tune camera_batches = 0), and checks what tests/test_gpu_camera_batches.py checks: both
frames are the CPU oracle's bit for bit (accumulator and rgba8) and each other's, segments and
samples of stats() are equal and the oracle's, and the tile-cost records are equal (every launch here
has fewer than 8 samples per unit, so the unit loop cannot split a unit). Bands are at most 64 x 40
at 8 spp or fewer.

Colours: a HASH launch, the only kind the form runs, is refused unless every colour a shader can
return as attenuation lies in [0, 1] (colours_in_unit), so a NaN, an infinity or a value above 1
never reaches a rebuilt thr; test_hash_refuses_a_colour_above_one pins that, and the "colours" scene
holds a value above 1 where the library accepts one: in colors[1] of an untextured sphere, which no
shader reads (alt = 0 there, and the rebuilt thr must be colors[0])."""
import numpy as np
import pytest

from test_gpu_camera_batches import both_forms, canon, check, small_only
from test_gpu_parity import HASH, LBVH, gpu_render  # noqa: F401
from test_gpu_parity import renderer, rtvk, torch  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu

DIFFUSE, METAL, DIELECTRIC = 0, 1, 2
SOLID, CHECKER = 0, 1
DENORMAL = np.float32(1e-40)
assert 0.0 < float(DENORMAL) < float(np.finfo(np.float32).tiny)


def sphere(x, y, z, r, mtype, ttype, c0, c1=(0.0, 0.0, 0.0), attr=0.0):
    """One 80-byte sphere record (include/rt_abi.h Sphere)."""
    rec = np.zeros((1, 80), np.uint8)
    rec[0, 0:16].view(np.float32)[:] = [x, y, z, r]
    rec[0, 16:24].view(np.uint32)[:] = [mtype, ttype]
    rec[0, 32:44].view(np.float32)[:] = c0
    rec[0, 48:60].view(np.float32)[:] = c1
    rec[0, 64:68].view(np.float32)[:] = [attr]
    return rec


def patch(kinds, n=11, step=0.9):
    """n x n small spheres of radius 0.2 in one layer around the look-at point, kinds[k] = (mtype,
    ttype, c0, c1, attr) dealt in turn."""
    recs, k = [], 0
    for i in range(-(n // 2), n // 2 + 1):
        for j in range(-(n // 2), n // 2 + 1):
            m, t, c0, c1, a = kinds[k % len(kinds)]
            recs.append(sphere(float(i) * step, 0.2, float(j) * step, 0.2, m, t, c0, c1, a))
            k += 1
    return np.concatenate(recs)


def every_material(oracle):
    """The canonical scene's ground (checkered) and three big spheres, the first of them a checkered
    dielectric, over a patch of small spheres of every material kind, solid and checkered."""
    sc = oracle.generate_scene()[:4].copy()
    big = sc[1]
    big[16:24].view(np.uint32)[:] = [DIELECTRIC, CHECKER]
    big[32:44].view(np.float32)[:] = [0.9, 0.8, 0.7]
    big[48:60].view(np.float32)[:] = [0.2, 0.3, 0.4]
    big[64:68].view(np.float32)[:] = [1.5]
    kinds = [(DIFFUSE, SOLID, (0.8, 0.3, 0.2), (0.1, 0.9, 0.1), 0.0),
             (DIFFUSE, CHECKER, (0.7, 0.6, 0.1), (0.1, 0.2, 0.9), 0.0),
             (METAL, SOLID, (0.9, 0.9, 0.5), (0.3, 0.3, 0.3), 0.3),
             (METAL, CHECKER, (0.6, 0.9, 0.9), (0.9, 0.2, 0.6), 0.0),
             (DIELECTRIC, SOLID, (1.0, 0.95, 0.9), (0.5, 0.5, 0.5), 1.5),
             (DIELECTRIC, CHECKER, (0.95, 1.0, 0.9), (0.4, 0.1, 0.7), 1.3)]
    return np.concatenate([sc, patch(kinds)])


def colours(oracle):
    """The checkered ground over a patch whose colours are 0, -0.0, a denormal and 1, in colors[0]
    and in a checker's colors[1]; an untextured sphere's unread colors[1] holds a value above 1."""
    z, nz, dn = 0.0, -0.0, float(DENORMAL)
    kinds = [(DIFFUSE, SOLID, (z, nz, dn), (2.5, 7.0, 1.5), 0.0),
             (DIFFUSE, CHECKER, (dn, z, nz), (nz, dn, z), 0.0),
             (METAL, SOLID, (nz, dn, 1.0), (3.0, 3.0, 3.0), 0.0),
             (METAL, CHECKER, (1.0, dn, dn), (dn, nz, 1.0), 0.1),
             (DIELECTRIC, CHECKER, (dn, 1.0, nz), (z, z, dn), 1.5),
             (DIFFUSE, SOLID, (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 0.0)]
    return np.concatenate([oracle.generate_scene()[:1], patch(kinds)])


LOOK_AT_IN_LAYER = (13.0 * 0.2 / 11.0, 0.2, -3.0 * 0.2 / 11.0)   # where the centre ray crosses y = 0.2


def full_table(oracle, last=True):
    """Exactly 512 spheres, the most a scene holds and the gate table's size: the ground, 510 small
    spheres on a lattice that leaves the centre ray's crossing of the layer free, and sphere 511
    there (last = False: far outside the view instead). That sphere 511 is a first hit is shown on
    the CPU, tests/test_batch_records_plan.py."""
    recs = [oracle.generate_scene()[:1]]
    for i in range(-15, 15):
        for j in range(-8, 9):
            recs.append(sphere(0.7 * i + 0.586, 0.2, 0.7 * j + 0.3, 0.2, (i + j) % 3, (i * j) & 1,
                               (0.8, 0.7, 0.6), (0.2, 0.3, 0.4), 1.5 if (i + j) % 3 == 2 else 0.2))
    x, y, z = LOOK_AT_IN_LAYER
    recs.append(sphere(x if last else x + 60.0, y, z, 0.2, DIFFUSE, SOLID, (1.0, 0.0, 0.0)))
    sc = np.concatenate(recs)
    assert len(sc) == 512
    return sc


def many_big(oracle):
    """The canonical scene and three more spheres of radius 1 in view: seven big spheres, so the
    second group of four takes the generic test."""
    sc = oracle.generate_scene()
    more = [sphere(2.0, 1.0, 2.5, 1.0, DIFFUSE, SOLID, (0.3, 0.6, 0.9)),
            sphere(-2.0, 1.0, -2.5, 1.0, METAL, SOLID, (0.8, 0.8, 0.8), attr=0.1),
            sphere(6.0, 1.0, -2.0, 1.0, DIELECTRIC, SOLID, (1.0, 1.0, 1.0), attr=1.5)]
    return np.concatenate([sc] + more)


ROWS = [0, 1, 5, 6, 7, 16, 17, 30, 31, 33, 39]
# name -> (scene, image W, H, offset, band_w, band_h, rows, spp, options)
CASES = {
    "canonical_64x40": (canon, 64, 40, (0, 0), 64, 40, None, 4, {}),
    "canonical_ragged_61x35": (canon, 61, 35, (0, 0), 61, 35, None, 4, {}),
    "max_depth_1_no_survivors": (every_material, 64, 40, (0, 0), 64, 40, None, 4, {"max_depth": 1}),
    "max_depth_2_popped_segment_is_last": (every_material, 64, 40, (0, 0), 64, 40, None, 4, {"max_depth": 2}),
    "every_material_and_checker_colour": (every_material, 64, 40, (0, 0), 64, 40, None, 6, {}),
    "colours_zero_negzero_denormal": (colours, 64, 40, (0, 0), 64, 40, None, 6, {}),
    "512_spheres_highest_id_first_hit": (full_table, 64, 40, (0, 0), 64, 40, None, 4, {}),
    "seven_big_spheres": (many_big, 64, 40, (0, 0), 64, 40, None, 4, {}),
    "no_big_spheres": (small_only, 64, 40, (0, 0), 64, 40, None, 4, {}),
    "rows_map_not_contiguous": (every_material, 64, 40, (3, 0), 50, len(ROWS), ROWS, 5, {}),
}
_REF = {}


def reference(oracle, case):
    """The oracle's frame of a case, computed once."""
    if case not in _REF:
        scene, W, H, off, bw, bh, rows, spp, kw = CASES[case]
        rows_np = None if rows is None else np.asarray(rows, np.uint32)
        _REF[case] = oracle.render(scene(oracle), oracle.render_call_info(spp, W, H, off), bw, bh, rows=rows_np,
                                   opts=oracle.options(rng_mode=HASH, **kw))
    return _REF[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_form_equals_oracle_and_unit_loop(rtvk, renderer, torch, oracle, case):
    scene, W, H, off, bw, bh, rows, spp, kw = CASES[case]
    sc = scene(oracle)
    ref = reference(oracle, case)
    rows_np = None if rows is None else np.asarray(rows, np.uint32)
    res = both_forms(rtvk, renderer, torch, sc, oracle.render_call_info(spp, W, H, off), bw, bh, rows_np, {}, **kw)
    segments, samples = int(ref[2][0]), int(ref[2][1])
    if kw.get("max_depth") == 1:
        assert segments == samples          # every path ended at its camera segment
    else:
        assert segments > samples           # paths were queued and popped
    if kw.get("max_depth") == 2:
        assert segments <= 2 * samples
    check(res, ref, can_split=False)


def test_progressive_accumulation_with_sample_base(rtvk, renderer, torch, oracle):
    """accumulate with sample_base != 0 over two launches: samples 0..2, then 3..7 on top."""
    W, H = 64, 40
    sc = every_material(oracle)
    base = oracle.render(sc, oracle.render_call_info(3, W, H), W, H, opts=oracle.options(rng_mode=HASH))
    rci = oracle.render_call_info(5, W, H)
    ref = oracle.render(sc, rci, W, H, accum=base[0], opts=oracle.options(rng_mode=HASH, accumulate=1, sample_base=3))
    first = both_forms(rtvk, renderer, torch, sc, oracle.render_call_info(3, W, H), W, H, None, {})
    check(first, base, can_split=False)
    res = both_forms(rtvk, renderer, torch, sc, rci, W, H, None, {}, accum=first[0][0], accumulate=True, sample_base=3)
    check(res, ref, can_split=False)


def test_hash_refuses_a_colour_above_one(rtvk, renderer, torch, oracle):
    """A colour a shader can return above 1 never reaches the form: the HASH launch is refused."""
    sc = colours(oracle)
    sc[5, 32:36].view(np.float32)[:] = [1.5]
    with pytest.raises(rtvk.RtError):
        gpu_render(rtvk, renderer, torch, sc, oracle.render_call_info(1, 8, 8), 8, 8, accel=LBVH, rng_mode=HASH)
