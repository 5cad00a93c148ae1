"""The camera-batch form after the pass over its own code (csrc/rt_trace_batch.h
batch_segment): the hit record of a segment has no value in a lane that loaded none, the winner's gate
is judged where the record was loaded, and shading's defaults (sd, p) exist only where a lane reads
them. What shading takes from a record, for every kind of material, at every depth limit and for
the highest sphere id, must be what it took before.

Every case renders one launch twice, with the form (launch_info()["camera_batches"]) and with the
unit loop (rt_debug_tune camera_batches = 0), as tests/test_gpu_camera_batches.py does: both frames
are the CPU oracle's bit for bit and each other's, segments and samples are the oracle's, and the
tile-cost records (a pixel's chain counters) are the same array.
64 x 40 pixels, 8 spp in two chunks of 4 samples: a unit of fewer than 8 samples cannot be split by
the unit loop, so the records must be equal, and every tile is two blocks.

The materials scene's premise is shown on the CPU first (test_materials_premise, no GPU): the oracle's
closest hit of the very camera rays the launch traces names, for every kind of material a record
describes (diffuse, metal without and with fuzz, a solid dielectric with its kMatDielConst record, a
checkered dielectric, the checkered ground), a sphere of that kind as some sample's first hit."""
import numpy as np
import pytest

import denoise_sim
from test_gpu_batch_records import CHECKER, DIELECTRIC, DIFFUSE, LOOK_AT_IN_LAYER, METAL, SOLID, full_table, sphere
from test_gpu_camera_batches import both_forms, canon, check
from test_gpu_parity import HASH  # noqa: F401
from test_gpu_parity import renderer, rtvk, torch  # noqa: F401  (module fixtures)

W, H, SPP, CHUNKS = 64, 40, 8, 2
MISS = 0xffffffff

# kind -> (mtype, ttype, colors[0], colors[1], attribute); a solid dielectric is the record with
# kMatDielConst (rt_internal.h make_mat), a checkered one computes its constants in the shader
KINDS = {
    "diffuse": (DIFFUSE, SOLID, (0.8, 0.3, 0.2), (0.0, 0.0, 0.0), 0.0),
    "metal_fuzz_0": (METAL, SOLID, (0.9, 0.9, 0.5), (0.0, 0.0, 0.0), 0.0),
    "metal_fuzz": (METAL, SOLID, (0.6, 0.9, 0.9), (0.0, 0.0, 0.0), 0.3),
    "dielectric_solid": (DIELECTRIC, SOLID, (1.0, 0.95, 0.9), (0.0, 0.0, 0.0), 1.5),
    "dielectric_checker": (DIELECTRIC, CHECKER, (0.95, 1.0, 0.9), (0.4, 0.1, 0.7), 1.3),
}
NAMES = sorted(KINDS)


def materials(oracle):
    """512 spheres, the gate table's size: the canonical checkered ground (id 0), 510 small spheres
    on test_gpu_batch_records.full_table's lattice with the five kinds dealt in turn (sphere k is
    NAMES[(k - 1) % 5]), and a solid dielectric as id 511 where the centre ray crosses the layer."""
    recs = [oracle.generate_scene()[:1]]
    k = 1
    for i in range(-15, 15):
        for j in range(-8, 9):
            m, t, c0, c1, a = KINDS[NAMES[(k - 1) % 5]]
            recs.append(sphere(0.7 * i + 0.586, 0.2, 0.7 * j + 0.3, 0.2, m, t, c0, c1, a))
            k += 1
    x, y, z = LOOK_AT_IN_LAYER
    m, t, c0, c1, a = KINDS["dielectric_solid"]
    recs.append(sphere(x, y, z, 0.2, m, t, c0, c1, a))
    sc = np.concatenate(recs)
    assert len(sc) == 512
    return sc


def kind_of(k):
    return "ground" if k == 0 else "dielectric_solid" if k == 511 else NAMES[(k - 1) % 5]


def test_materials_premise(oracle):
    """No GPU: the first hits of the launch's own camera rays (samples 0..7 of every pixel of the
    64 x 40 frame, the counter-based stream) hold the checkered ground and a sphere of every kind,
    id 511 among them, and the ground's record is a checker."""
    sc = materials(oracle)
    assert tuple(sc[0, 16:24].view(np.uint32)) == (DIFFUSE, CHECKER)
    rays = denoise_sim.camera_rays(oracle, oracle.render_call_info(SPP, W, H), W, H, SPP)
    ids, _ = oracle.closest_hits(sc, rays.reshape(-1, 6))
    first = {kind_of(int(k)) for k in np.unique(ids) if k != MISS}
    assert first == set(NAMES) | {"ground"}, first
    assert 511 in ids


# name -> (scene, options)
CASES = {
    "canonical_depth_50": (canon, {}),
    "canonical_depth_2": (canon, {"max_depth": 2}),
    "canonical_depth_1": (canon, {"max_depth": 1}),
    "512_spheres_highest_id_first_hit": (full_table, {}),
    "every_material_in_a_full_table": (materials, {}),
}
_REF = {}


def reference(oracle, case):
    """The oracle's frame of a case, computed once."""
    if case not in _REF:
        scene, kw = CASES[case]
        _REF[case] = oracle.render(scene(oracle), oracle.render_call_info(SPP, W, H), W, H,
                                   opts=oracle.options(rng_mode=HASH, **kw))
    return _REF[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_form_equals_oracle_and_unit_loop(rtvk, renderer, torch, oracle, case):
    scene, kw = CASES[case]
    ref = reference(oracle, case)
    res = both_forms(rtvk, renderer, torch, scene(oracle), oracle.render_call_info(SPP, W, H), W, H, None,
                     {"sample_chunks": CHUNKS}, **kw)
    assert renderer.launch_info()["chunks"] == CHUNKS
    segments, samples = int(ref[2][0]), int(ref[2][1])
    assert samples == W * H * SPP
    assert segments == samples if kw.get("max_depth") == 1 else segments > samples
    check(res, ref, can_split=False)   # (the tile-cost records are compared there)
    assert res[0][3].any()             # ... and hold a record
