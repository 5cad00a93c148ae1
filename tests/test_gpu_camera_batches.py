"""The camera-batch form of the LDS grid kernel (csrc/rt_trace_batch.h) on the GPU.
Every case renders the same launch twice, with the form (the default; launch_info()["camera_batches"])
and with the unit loop (rt_debug_tune camera_batches = 0), and checks three things: both frames are
the CPU oracle's bit for bit (accumulator and rgba8); the two frames are each other's; segments and
samples of stats() are equal and the oracle's, and the tile-cost record the next launch's hand-out
order is made from is the same. (The unit loop splits a pixel's last samples between idle lanes once
the work queue is dry, and a split unit records only its own part of the chain, so its record can
only be smaller; a launch whose units hold fewer than 8 samples cannot split and must be equal.)"""
import numpy as np
import pytest

from test_gpu_parity import HASH, LBVH, assert_same, gpu_render, tuned  # noqa: F401
from test_gpu_parity import renderer, rtvk, torch  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu


def canon(oracle):
    return oracle.generate_scene()


def with_dielectric_ball(oracle):
    """The canonical scene and one glass sphere of radius 2 between the camera and the scene, 3.5
    from the camera: most camera rays enter it and bounce inside."""
    sc = oracle.generate_scene()
    glass = sc[np.flatnonzero(sc[:, 16:20].copy().view(np.uint32)[:, 0] == 2)[:1]].copy()
    assert len(glass) == 1
    glass[0, :16].view(np.float32)[:] = [10.4, 8.8, -2.4, 2.0]
    return np.concatenate([sc, glass])


def small_only(oracle):
    """11 x 11 small spheres in one layer, no ground and no other big sphere."""
    base = oracle.generate_scene()[4:5]
    recs = []
    for i in range(-5, 6):
        for j in range(-5, 6):
            r = base.copy()
            r[0, :16].view(np.float32)[:] = [float(i) * 0.9, 0.2, float(j) * 0.9, 0.2]
            recs.append(r)
    return np.concatenate(recs)


def out_of_view(oracle):
    """small_only moved 400 along x, behind the camera: every camera ray ends in the sky."""
    sc = small_only(oracle)
    for r in sc:
        r[:4].view(np.float32)[0] += 400.0
    return sc


# name -> (scene, image W, H, offset, band_w, band_h, rows, spp, options, tuning)
CASES = {
    "one_block_one_batch": (canon, 8, 8, (0, 0), 8, 8, None, 1, {}, {}),
    "fewer_tiles_than_waves": (canon, 24, 16, (0, 0), 24, 16, None, 3, {}, {}),
    "ragged_edges": (canon, 17, 9, (0, 0), 17, 9, None, 5, {}, {}),
    "two_waves_share_a_tile": (canon, 16, 16, (0, 0), 16, 16, None, 130, {}, {"sample_chunks": 3}),
    "every_path_ends_in_the_batch": (canon, 24, 16, (0, 0), 24, 16, None, 4, {"max_depth": 1}, {}),
    "long_paths": (with_dielectric_ball, 24, 16, (0, 0), 24, 16, None, 24, {"max_depth": 50}, {}),
    "nothing_enters_the_queue": (out_of_view, 24, 16, (0, 0), 24, 16, None, 3, {}, {}),
    "no_big_spheres": (small_only, 24, 16, (0, 0), 24, 16, None, 3, {}, {}),
    "rows_map_and_offset": (canon, 40, 40, (5, 0), 24, 9, [3, 4, 10, 11, 12, 20, 21, 30, 31], 3, {}, {}),
}


def both_forms(rtvk, renderer, torch, sc, rci, bw, bh, rows, tune, **kw):
    """The launch with the form and with the unit loop: ((accum, rgba8, stats, tile costs) x 2)."""
    res = []
    for batches in (None, 0):
        with tuned(renderer, camera_batches=batches, **tune):
            a, o, st = gpu_render(rtvk, renderer, torch, sc, rci, bw, bh, rows=rows, accel=LBVH, rng_mode=HASH, **kw)
            info = renderer.launch_info()
            assert info["form"] == "grid-lds-rec" and info["flat_grid"] and info["pinhole_origin"]
            assert info["camera_batches"] == (batches is None)
            res.append((a, o, st, renderer.tile_costs().copy()))
    return res


def check(res, ref, can_split):
    (a, o, st, cost), (a0, o0, st0, cost0) = res
    ra, ro, rs = ref
    assert_same(a, o, ra, ro)
    assert_same(a0, o0, ra, ro)
    assert_same(a, o, a0, o0)
    print(f"segments {st.segments} / {st0.segments} / {rs[0]}, samples {st.samples} / {st0.samples} / {rs[1]}")
    assert (st.segments, st.samples) == (st0.segments, st0.samples) == tuple(int(v) for v in rs[:2])
    assert cost.shape == cost0.shape
    if can_split:
        assert np.all(cost >= cost0) and cost.max() >= cost0.max()
    else:
        np.testing.assert_array_equal(cost, cost0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_form_equals_oracle_and_unit_loop(rtvk, renderer, torch, oracle, case):
    scene, W, H, off, bw, bh, rows, spp, kw, tune = CASES[case]
    sc = scene(oracle)
    rci = oracle.render_call_info(spp, W, H, off)
    rows_np = None if rows is None else np.asarray(rows, np.uint32)
    ref = oracle.render(sc, rci, bw, bh, rows=rows_np, opts=oracle.options(rng_mode=HASH, **kw))
    res = both_forms(rtvk, renderer, torch, sc, rci, bw, bh, rows_np, tune, **kw)
    if case == "two_waves_share_a_tile":
        assert renderer.launch_info()["chunks"] == 3
    if case == "nothing_enters_the_queue":
        assert ref[2][0] == ref[2][1]   # one segment per sample: every path ended at its camera segment
    check(res, ref, can_split=spp // max(1, tune.get("sample_chunks", 1)) >= 8)


def test_progressive_accumulation(rtvk, renderer, torch, oracle):
    """accumulate with sample_base != 0 over two launches: samples 0..2, then 3..7 on top."""
    W, H = 24, 16
    sc = canon(oracle)
    base = oracle.render(sc, oracle.render_call_info(3, W, H), W, H, opts=oracle.options(rng_mode=HASH))
    rci = oracle.render_call_info(5, W, H)
    ref = oracle.render(sc, rci, W, H, accum=base[0], opts=oracle.options(rng_mode=HASH, accumulate=1, sample_base=3))
    first = both_forms(rtvk, renderer, torch, sc, oracle.render_call_info(3, W, H), W, H, None, {})
    check(first, base, can_split=False)
    res = both_forms(rtvk, renderer, torch, sc, rci, W, H, None, {}, accum=first[0][0], accumulate=True, sample_base=3)
    check(res, ref, can_split=False)


def test_second_launch_consumes_the_first_launchs_order(rtvk, renderer, torch, oracle):
    """A launch followed by a second one of the same band: the second hands its tiles out in the LPT
    order made from the first launch's tile costs (the plan's lpt flag), with the form and without,
    and renders the same bits."""
    W, H, spp = 40, 24, 6
    sc = canon(oracle)
    rci = oracle.render_call_info(spp, W, H)
    ref = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=HASH))
    for batches in (None, 0):
        with tuned(renderer, camera_batches=batches):
            frames = []
            for k in range(2):
                a, o, st = gpu_render(rtvk, renderer, torch, sc, rci, W, H, accel=LBVH, rng_mode=HASH)
                assert renderer.launch_info()["camera_batches"] == (batches is None)
                frames.append((a, o, st, renderer.tile_costs().copy()))
            assert renderer.launch_plan()[1].lpt == 1
        for a, o, st, cost in frames:
            assert_same(a, o, ref[0], ref[1])
            assert (st.segments, st.samples) == tuple(int(v) for v in ref[2][:2])
        np.testing.assert_array_equal(frames[0][3], frames[1][3])
