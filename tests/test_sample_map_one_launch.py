"""Sample-map frames under the one-launch schedule (RT_SAMPLE_MAP_ONE_LAUNCH) on the
GPU: the whole frame is one trace launch whose blocks come from a table {tile, s0, s1}. The standard
of proof is tests/test_sample_map.py's: every texel equals adaptive_sim.expected_frame(oracle, counts)
on every accumulator float and rgba8 byte and the per-texel count equals the table, with the output
buffers pre-filled with sentinels. Shapes and helpers are that file's.

What can go wrong here and the case that shows it: a table entry read for the wrong block (units of
1, 3 and 5 samples: uneven chunk splits, one block per sample), the two hand-out phases and their
boundary (refill_reserve 0, 640 and the default), a ragged width and a ragged last tile row, zero
tiles (absent from the table), more than 64 distinct counts, a rows map with a sample base."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
from test_sample_map import (AUTO, BRUTE, EXAMPLE, HASH, MAX, ROWS, TABLE_64x40, adaptive_parity, assert_exact, lib,   # noqa: E402
                             plain_exact, queue_map_frame, rci_of, renderer, sentinels, set_map, table_for, texel_counts,
                             to_host, torch)

__all__ = ["lib", "renderer", "torch"]   # the fixtures of tests/test_sample_map.py, module-scoped here too
LEVELS, ONE = 0, 1
TABLE_71 = [1 + (29 * t) % 71 for t in range(72)]   # 9 x 8 tiles, 71 distinct counts


def one_launch_parity(lib, renderer, torch, oracle, W, H, table, unit=0, quantum=0, k=11, set_scene=True, **kw):
    """One frame of `table` under ONE_LAUNCH with units of `unit` samples against the oracle. Returns
    (the set call's info, the map's schedule_info). `k`: the scene's key in adaptive_sim; `options` (in
    kw): ready-made rt_options, see test_sample_map.frame_options."""
    if set_scene:
        renderer.set_scene(sim.scene(oracle, k))
    q = max(1, quantum)
    quantised = (np.asarray(table, np.int64) + q - 1) // q * q
    counts = texel_counts(quantised, W, H)
    sk = {key: kw[key] for key in ("rows", "base", "image") if key in kw}
    ref = sim.expected_frame(oracle, counts, k=k, **sk)
    with renderer.sample_map(W, H) as smap:
        smap.schedule(ONE, unit)
        info = set_map(torch, smap, table, quantum)
        sched = smap.schedule_info()
        bufs = queue_map_frame(lib, renderer, torch, oracle, smap, W, H, **kw)
        torch.cuda.synchronize()
        assert_exact(to_host(bufs), counts, ref)
    assert info.samples == int(counts.astype(np.int64).sum()) and info.tiles == len(table)
    assert info.tile_launches == int((quantised > 0).sum()) and info.levels == len(np.unique(quantised[quantised > 0]))
    want = lib.sample_map_block_plan(table, quantum, unit)
    assert sched == {"schedule": ONE, "unit_samples": want["unit_samples"], "n_blocks": len(want["blocks"])}
    return info, sched


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [0, 1, 3, 5])
@pytest.mark.parametrize("accel", [BRUTE, AUTO])
@pytest.mark.parametrize("shape", [(44, 27), (64, 40)])
def test_parity(lib, renderer, torch, oracle, shape, accel, unit):
    info, sched = one_launch_parity(lib, renderer, torch, oracle, *shape, table_for(*shape), unit=unit, accel=accel)
    assert sched["unit_samples"] == (unit or 32)
    if unit == 1:
        assert sched["n_blocks"] == sum(table_for(*shape))   # one block per sample of a tile


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [0, 640])
def test_block_phase_and_its_boundary(lib, renderer, torch, oracle, reserve):
    """64x40 at U = 3: 203 blocks, 12 992 units (then 44x27 at U = 1: 319 blocks). By default the last
    8 192 units go out one by one, which is all of most frames of test_parity; reserve 0 hands every
    unit out by blocks (the waves' first blocks by wave id, the rest through the counter), reserve 640
    puts the boundary inside the table."""
    renderer.tune(refill_reserve=reserve)
    try:
        _, sched = one_launch_parity(lib, renderer, torch, oracle, 64, 40, TABLE_64x40, unit=3)
        assert sched["n_blocks"] == 203
        one_launch_parity(lib, renderer, torch, oracle, 44, 27, EXAMPLE, unit=1, accel=BRUTE, set_scene=False)
    finally:
        renderer.tune(refill_reserve=None)


@pytest.mark.gpu
def test_more_than_64_levels(lib, renderer, torch, oracle):
    from rtvk import RtError
    W, H = 68, 60   # 9 x 8 tiles, ragged both ways
    renderer.set_scene(sim.scene(oracle))
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, [2] * 72)
        with pytest.raises(RtError) as e:
            set_map(torch, smap, TABLE_71)      # the level schedule refuses 71 levels ...
        assert e.value.code == -1 and "71 levels" in str(e.value)
        assert (smap.info.levels, smap.info.max_count) == (1, 2)   # ... and the map keeps what it held
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H, cap=71))
        counts = texel_counts([2] * 72, W, H)
        assert_exact(got, counts, sim.expected_frame(oracle, counts))
    info, _ = one_launch_parity(lib, renderer, torch, oracle, W, H, TABLE_71, cap=71, set_scene=False)
    assert (info.levels, info.min_count, info.max_count, info.tile_launches) == (71, 1, 71, 72)


@pytest.mark.gpu
def test_the_two_schedules_agree(lib, renderer, torch, oracle):
    """The device-built 1 160-sphere scene (its L2 grid / treelet walks): accumulator, rgba8 and counts
    of the same map under either schedule, bit for bit (and both against the oracle)."""
    W, H = 44, 27
    renderer.set_scene(sim.scene(oracle, 17))
    assert renderer.scene_array(8)["device_built"]
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, EXAMPLE)
        a = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        smap.schedule(ONE, 5)
        set_map(torch, smap, EXAMPLE)
        b = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    counts = texel_counts(EXAMPLE, W, H)
    assert_exact(b, counts, sim.expected_frame(oracle, counts, k=17))


@pytest.mark.gpu
def test_rows_map_and_sample_base(lib, renderer, torch, oracle):
    """Non-contiguous rows of a 44x40 image and sample_base = 1000: a band of a larger image."""
    one_launch_parity(lib, renderer, torch, oracle, 44, len(ROWS), EXAMPLE[:18], unit=5, rows=ROWS, base=1000,
                      image=(44, 40))


@pytest.mark.gpu
def test_replay_of_an_adaptive_frame(lib, renderer, torch, oracle):
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    counts, (acc_a, out_a, cnt_a), info_a = adaptive_parity(lib, renderer, torch, oracle, W, H)
    with renderer.sample_map(W, H) as smap:
        smap.schedule(ONE)
        info = smap.set_from_adaptive(0)
        assert info.samples == info_a.samples and info.tiles == info_a.tiles == 40
        assert info.tile_launches == 40 and info.levels == len(np.unique(counts))
        np.testing.assert_array_equal(smap.debug_blocks(), lib.sample_map_block_plan(counts[::8, ::8].ravel())["blocks"])
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert np.array_equal(acc, acc_a) and np.array_equal(out, out_a) and np.array_equal(cnt, cnt_a)


@pytest.mark.gpu
def test_records(lib, torch, oracle):
    W, H = 44, 27
    with lib.Renderer(0) as r:   # a fresh context: its launch ring starts empty
        r.set_scene(sim.scene(oracle))
        assert len(r.kernel_times()) == 0
        with r.sample_map(W, H) as smap:
            assert smap.schedule_info() == {"schedule": LEVELS, "unit_samples": 0, "n_blocks": 0}
            launches = 0
            for quantum, unit in ((0, 0), (16, 5), (0, 3)):
                smap.schedule(ONE, unit)
                info = set_map(torch, smap, EXAMPLE, quantum)
                want = lib.sample_map_block_plan(EXAMPLE, quantum, unit)
                np.testing.assert_array_equal(smap.debug_blocks(), want["blocks"])
                assert smap.schedule_info() == {"schedule": ONE, "unit_samples": want["unit_samples"],
                                                "n_blocks": len(want["blocks"])}
                queue_map_frame(lib, r, torch, oracle, smap, W, H)
                torch.cuda.synchronize()
                launches += 1   # a frame is exactly one trace launch
                times = r.kernel_times()
                assert len(times) == launches and all(t > 0 for t in times)
                assert r.launch_ms(0) == times[-1]
            # the instrumented build counts the samples of the last launch: the whole frame
            bufs = sentinels(torch, W, H)
            r.render_sample_map(rci_of(lib, oracle, MAX, W, H), bufs[0], bufs[1], smap, sample_count=bufs[2],
                                options=lib.make_options(rng_mode=HASH, count_tests=True))
            torch.cuda.synchronize()
            assert r.stats().samples == info.samples == int(texel_counts(EXAMPLE, W, H).astype(np.int64).sum())
            assert len(r.kernel_times()) == launches + 1
            counts = texel_counts(EXAMPLE, W, H)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts))


@pytest.mark.gpu
def test_hygiene(lib, renderer, torch, oracle):
    """Frames back to back on one map, the schedule switched LEVELS -> ONE_LAUNCH -> LEVELS between
    them, a plain frame before and after (the planes are left zero), the uniform and the all-zero map,
    and the last adaptive frame's count table survives."""
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    counts_a, got_a, _ = adaptive_parity(lib, renderer, torch, oracle, W, H)
    pa, po = plain_exact(lib, renderer, torch, oracle, W, H, 6)
    other = TABLE_64x40[::-1]
    with renderer.sample_map(W, H) as smap:
        frames = []
        set_map(torch, smap, TABLE_64x40)                       # LEVELS
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), TABLE_64x40))
        smap.schedule(ONE, 3)
        assert smap.schedule_info()["schedule"] == LEVELS       # takes effect at the next set call
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), TABLE_64x40))
        set_map(torch, smap, other)                             # ONE_LAUNCH
        assert smap.schedule_info()["schedule"] == ONE
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), other))
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), other))
        smap.schedule(LEVELS)
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), other))
        set_map(torch, smap, TABLE_64x40)                       # LEVELS again
        assert smap.schedule_info() == {"schedule": LEVELS, "unit_samples": 0, "n_blocks": 0}
        assert smap.debug_blocks().shape == (0, 4)
        frames.append((queue_map_frame(lib, renderer, torch, oracle, smap, W, H), TABLE_64x40))
        torch.cuda.synchronize()
        for bufs, table in frames:
            counts = texel_counts(table, W, H)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts))
        qa, qo = plain_exact(lib, renderer, torch, oracle, W, H, 6)
        assert np.array_equal(pa, qa) and np.array_equal(po, qo)
        # the uniform map is the plain frame, the all-zero map the 0-sample frame (the resolve alone)
        smap.schedule(ONE)
        info = set_map(torch, smap, [6] * 40)
        assert (info.levels, info.tile_launches, info.samples) == (1, 40, 6 * W * H)
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert np.array_equal(acc, pa) and np.array_equal(out, po) and (cnt == 6).all()
        info = set_map(torch, smap, [0] * 40)
        assert (info.levels, info.tile_launches, info.samples, info.max_count) == (0, 0, 0, 0)
        assert smap.schedule_info() == {"schedule": ONE, "unit_samples": 32, "n_blocks": 0}
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert (acc == np.array([0, 0, 0, 1], np.float32)).all() and (out == np.array([0, 0, 0, 255], np.uint8)).all()
        assert (cnt == 0).all()
        # the last adaptive frame's count table is still in place
        info = smap.set_from_adaptive(0)
        np.testing.assert_array_equal(smap.debug_plan()["quantised"], counts_a[::8, ::8].ravel())
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert np.array_equal(acc, got_a[0]) and np.array_equal(out, got_a[1]) and np.array_equal(cnt, got_a[2])


@pytest.mark.gpu
def test_refusals(lib, renderer, torch, oracle):
    from rtvk import RtError, abi
    W, H = 44, 27
    renderer.set_scene(sim.scene(oracle))
    acc, out, cnt = sentinels(torch, W, H)

    def refused(field, call):
        with pytest.raises(RtError) as e:
            call()
        assert e.value.code == -1 and field in str(e.value), str(e.value)   # RT_ERR_INVALID_ARGUMENT

    def render(smap, spp=MAX, **opt):
        o = dict(rng_mode=HASH)
        o.update(opt)
        renderer.render_sample_map(rci_of(lib, oracle, spp, W, H), acc, out, smap, sample_count=cnt,
                                   options=lib.make_options(**o))

    with renderer.sample_map(W, H) as smap, renderer.sample_map(64, 40) as big:
        smap.schedule(ONE, 3)
        set_map(torch, smap, EXAMPLE)
        held = smap.schedule_info()
        refused("unknown schedule", lambda: smap.schedule(2))
        refused("unit_samples", lambda: smap.schedule(LEVELS, 5))
        refused("2^19", lambda: smap.schedule(ONE, (1 << 19) + 1))
        assert lib.load_library().rt_sample_map_set_schedule(None, ONE, 0) == -1      # a NULL map
        assert lib.load_library().rt_sample_map_get_schedule(None, None, None, None) == -1
        bad = list(EXAMPLE)
        bad[7] = (1 << 19) + 1
        refused("tile_counts[7]", lambda: set_map(torch, smap, bad))
        assert smap.schedule_info() == held and smap.info.levels == 10   # the refusals left the map as it was
        np.testing.assert_array_equal(smap.debug_blocks(), lib.sample_map_block_plan(EXAMPLE, 0, 3)["blocks"])
        big.schedule(ONE)
        set_map(torch, big, TABLE_64x40)
        # the render call's own refusals under the new schedule
        refused("rng_mode", lambda: render(smap, rng_mode=abi.RT_RNG_PIXEL_STREAM))
        refused("rng_mode", lambda: render(smap, rng_mode=abi.RT_RNG_SAMPLE_COUNTER))
        refused("accumulate", lambda: render(smap, accumulate=True))
        refused("samplesPerRenderCall", lambda: render(smap, spp=63))   # the cap below the map's max_count
        refused("band size", lambda: render(big))                        # a 64x40 map for 44x27 buffers
        torch.cuda.synchronize()
        assert float((acc + 1.0).abs().sum()) == 0.0 and int((out != 7).sum()) == 0 and int((cnt != -1).sum()) == 0
        # afterwards a clean frame
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        counts = texel_counts(EXAMPLE, W, H)
        assert_exact(got, counts, sim.expected_frame(oracle, counts))
