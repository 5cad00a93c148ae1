"""The camera-batch form's LDS after its queue entry lost its thr (csrc/rt_internal.h
kBatchLdsBytes), on the CPU: the bytes rt_debug_camera_batches reports for the kernel are what they
were, now made of other parts; and two premises of tests/test_gpu_batch_records.py, by the oracle:
the canonical tile list holds generation batches with 64 survivors and with none, and the
512-sphere scene's highest id is a first hit."""
import numpy as np

from test_camera_batches_plan import decide
from test_gpu_batch_records import full_table
from test_launch_plan import rtvk  # noqa: F401  (module fixture)

HASH = 2


def test_static_lds_is_still_55408(rtvk):
    d, plan = decide(rtvk)
    assert d["on"]
    sums, queue, chains, gate, camera_terms, walk_params = 3 * 8 * 768, 2 * 16 * 768, 4 * 768, 16 * 512, 1024, 112
    assert queue + chains + gate + camera_terms == 36864
    assert d["static_lds"] == sums + queue + chains + gate + camera_terms + walk_params == 55408
    assert d["lds_total"] == 55408 + plan["lds"] <= 78 * 1024


def survivors(oracle, sc, W, H, tile, s, max_depth):
    """Paths of the generation batch (tile, sample s) that enter the queue, by the form's own
    path-end condition (shade_rec: the camera segment scattered and depth 1 < max_depth): each
    traces a second segment when max_depth >= 2, so at max_depth <= 2 they are the segments beyond
    one per sample."""
    tx, ty = tile % (W // 8), tile // (W // 8)
    rows = np.arange(ty * 8, ty * 8 + 8, dtype=np.uint32)
    _, _, st = oracle.render(sc, oracle.render_call_info(1, W, H, (tx * 8, 0)), 8, 8, rows=rows,
                             opts=oracle.options(rng_mode=HASH, max_depth=min(max_depth, 2), sample_base=s))
    assert int(st[1]) == 64
    return int(st[0]) - 64


def test_canonical_batches_have_64_survivors_and_none(oracle):
    """The canonical 64 x 40 frame's tile list (40 tiles of 8 x 8), samples 0 and 1, at the depths
    the GPU cases use. Every camera ray of the canonical view hits the ground or a sphere, so the
    full queue is the rule; the empty one comes from the depth limit (max_depth = 1)."""
    sc = oracle.generate_scene()
    W, H = 64, 40
    counts = {(tile, s, depth): survivors(oracle, sc, W, H, tile, s, depth)
              for tile in range((W // 8) * (H // 8)) for s in (0, 1) for depth in (1, 2, 50)}
    assert all(0 <= n <= 64 for n in counts.values())
    assert any(n == 64 for n in counts.values())
    assert any(n == 0 for n in counts.values())
    assert all(n == 0 for (_, _, depth), n in counts.items() if depth == 1)


def test_sphere_511_is_a_first_hit(oracle):
    """Sphere 511 is diffuse red, (1, 0, 0). At max_depth 2 a sample adds its first hit's colour
    times the sky's where the bounce escapes and nothing otherwise, so a pixel whose sum has red and
    neither green nor blue hit sphere 511 first; no other colour of the scene lacks both. With the
    sphere moved out of view there is no such pixel."""
    W, H, spp = 64, 40, 8
    opts = oracle.options(rng_mode=HASH, max_depth=2)
    a = oracle.render(full_table(oracle), oracle.render_call_info(spp, W, H), W, H, opts=opts)[0]
    b = oracle.render(full_table(oracle, last=False), oracle.render_call_info(spp, W, H), W, H, opts=opts)[0]

    def red(f):
        return (f[..., 0] > 0) & (f[..., 1] == 0) & (f[..., 2] == 0)
    assert red(a).any() and not red(b).any()
