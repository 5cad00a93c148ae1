"""Sample maps planned on the device (rt_sample_map_set_device_async) on the GPU.

The planner alone: after set_async the block table the device holds equals, word for word, the host
planner's table of the clamped counts at the unit the host twin (rt_sample_map_device_unit) names;
so do the order and the clamped table, and the summary's totals. The cases are those in which a
sort, a scan or an expansion goes wrong: zeros, ones, odd counts, ties (tile order), a count at the
cap, counts above it (one by one, and 2^32 - 1), more than 64 distinct counts, units of 1, 3 and 128
samples and the automatic one, a capacity that forces one doubling of the unit and one that forces
several. Bands ragged both ways.

The launch: the trace kernels take the table's size from a device record and run on the full
persistent grid. Every frame is compared in every texel with adaptive_sim.expected_frame, and bit for
bit with the frame of the same table set synchronously; the size-record cases are the empty table, a
one-block table and the 203-block table at the three hand-out boundaries of
test_sample_map_one_launch.py. Helpers and shapes are tests/test_sample_map.py's."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
from test_sample_map import (AUTO, BRUTE, EXAMPLE, HASH, MAX, ROWS, TABLE_64x40, assert_exact, lib, plain_exact,   # noqa: E402
                             queue_map_frame, renderer, rci_of, sentinels, set_map, texel_counts, to_host, torch)

__all__ = ["lib", "renderer", "torch"]   # the fixtures of tests/test_sample_map.py, module-scoped here too
ONE = 1
TABLE_71 = [1 + (29 * t) % 71 for t in range(72)]   # 9 x 8 tiles (68x60), 71 distinct counts
# 44x27 with counts above the cap: 65 (one above 64), 1000, and the largest word
OVER = [65 if t == 3 else 1000 if t == 10 else 0xffffffff if t == 20 else c for t, c in enumerate(EXAMPLE)]


def to_device(torch, table):
    return torch.from_numpy(np.asarray(table, np.int64).astype(np.uint32).view(np.int32)).cuda()


def check_plan(lib, smap, table, unit, cap, limit=0):
    """What the device holds after set_async against the host: unit, block table, order, clamped
    counts, summary. Returns (U, blocks)."""
    raw = np.asarray(table, np.int64)
    clamped = np.minimum(raw, cap)
    n = len(raw)
    capacity = lib.sample_map_device_capacity(n, cap, unit)
    if limit:
        capacity = min(capacity, max(limit, n))
    U = lib.sample_map_device_unit(raw, cap, unit, capacity)
    want = lib.sample_map_block_plan(clamped, 0, U)
    assert want["unit_samples"] == U and len(want["blocks"]) <= capacity
    got = smap.debug_blocks()
    assert got.shape == want["blocks"].shape
    np.testing.assert_array_equal(got, want["blocks"])
    assert smap.schedule_info() == {"schedule": ONE, "unit_samples": U, "n_blocks": len(want["blocks"])}
    plan = smap.debug_plan()
    np.testing.assert_array_equal(plan["quantised"], clamped)
    np.testing.assert_array_equal(plan["order"], np.lexsort((np.arange(n), -clamped)))   # count descending, tile ascending
    info = smap.info
    W, H = smap.width, smap.height
    assert (info.tiles, info.max_count, info.tile_launches) == (n, int(clamped.max(initial=0)), int((clamped > 0).sum()))
    assert info.samples == int(texel_counts(clamped, W, H).astype(np.int64).sum())
    return U, want["blocks"]


def async_parity(lib, renderer, torch, oracle, W, H, table, unit=0, cap=MAX, k=11, set_scene=True, limit=0, **kw):
    """set_async and one frame queued behind it without a wait, against the oracle at the clamped
    counts; then the plan. Returns (U, blocks, the frame)."""
    if set_scene:
        renderer.set_scene(sim.scene(oracle, k))
    counts = texel_counts(np.minimum(np.asarray(table, np.int64), cap), W, H)
    sk = {key: kw[key] for key in ("rows", "base", "image") if key in kw}
    ref = sim.expected_frame(oracle, counts, k=k, **sk)
    with renderer.sample_map(W, H) as smap:
        smap.debug_limit_blocks(limit)
        smap.set_async(to_device(torch, table), unit, cap)
        bufs = queue_map_frame(lib, renderer, torch, oracle, smap, W, H, cap=cap, **kw)
        torch.cuda.synchronize()
        got = to_host(bufs)
        assert_exact(got, counts, ref)
        U, blocks = check_plan(lib, smap, table, unit, cap, limit)
    return U, blocks, got


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [0, 1, 3, 128])
@pytest.mark.parametrize("shape,table", [((44, 27), EXAMPLE), ((44, 27), OVER), ((64, 40), TABLE_64x40)])
def test_planner_and_frame(lib, renderer, torch, oracle, shape, table, unit):
    U, blocks, _ = async_parity(lib, renderer, torch, oracle, *shape, table, unit=unit)
    assert U == (unit or 32)   # the map's own capacity holds every tile at the cap: no doubling
    if unit == 1:
        assert len(blocks) == int(np.minimum(np.asarray(table, np.int64), MAX).sum())   # one block per sample


@pytest.mark.gpu
def test_more_than_64_distinct_counts(lib, renderer, torch, oracle):
    U, blocks, _ = async_parity(lib, renderer, torch, oracle, 68, 60, TABLE_71, unit=5, cap=71)
    assert U == 5 and len(np.unique(blocks[:, 0])) == 72


@pytest.mark.gpu
def test_capacity_doubles_the_unit(lib, renderer, torch, oracle):
    """64x40 at U0 = 3 has 203 blocks; a capacity of 202 forces exactly one doubling, one of 40 (the
    tiles) several, and a cap below the counts clamps before anything is counted."""
    at = lambda u, cap=MAX: sum(-(-min(c, cap) // u) for c in TABLE_64x40)
    assert at(3) == 203 and at(6) <= 202
    U, blocks, _ = async_parity(lib, renderer, torch, oracle, 64, 40, TABLE_64x40, unit=3, limit=202)
    assert U == 6 and len(blocks) == at(6)
    U, blocks, _ = async_parity(lib, renderer, torch, oracle, 64, 40, TABLE_64x40, unit=3, limit=1, set_scene=False)
    fits = [3 << j for j in range(20) if at(3 << j) <= 40]
    assert U == fits[0] > 6 and at(U // 2) > 40 and len(blocks) == at(U)   # several doublings
    U, blocks, _ = async_parity(lib, renderer, torch, oracle, 64, 40, TABLE_64x40, unit=3, cap=30, limit=at(3, 30) - 1,
                                set_scene=False)
    assert U == 6 and int(blocks[:, 2].max()) == 30


@pytest.mark.gpu
@pytest.mark.parametrize("shape,table,unit", [((44, 27), EXAMPLE, 5), ((64, 40), TABLE_64x40, 0)])
def test_frame_equals_the_synchronous_set(lib, renderer, torch, oracle, shape, table, unit):
    """The same table set synchronously under ONE_LAUNCH at the same unit: the same block table, and
    accumulator, rgba8 and counts bit for bit."""
    W, H = shape
    U, blocks, got = async_parity(lib, renderer, torch, oracle, W, H, table, unit=unit)
    with renderer.sample_map(W, H) as smap:
        smap.schedule(ONE, U)
        set_map(torch, smap, table)
        np.testing.assert_array_equal(smap.debug_blocks(), blocks)
        want = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [0, 640, None])
def test_size_record(lib, renderer, torch, oracle, reserve):
    """The sizes of the launch come from device memory and the grid is the full persistent grid: an
    empty table (0 blocks: every wave retires at once, the frame is the 0-sample frame), a one-tile
    table (1 block, below the grid's waves; below the one-by-one reserve unless that is 0) and the
    203-block table, with the block phase's boundary at 0, inside the table and beyond it."""
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    renderer.tune(refill_reserve=reserve)
    try:
        with renderer.sample_map(W, H) as smap:
            smap.set_async(to_device(torch, [0] * 40), 3, MAX)
            acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
            assert (acc == np.array([0, 0, 0, 1], np.float32)).all() and (out == np.array([0, 0, 0, 255], np.uint8)).all()
            assert (cnt == 0).all()
            assert smap.schedule_info() == {"schedule": ONE, "unit_samples": 3, "n_blocks": 0}
            assert smap.debug_blocks().shape == (0, 4)
            one = [0] * 40
            one[13] = 2
            smap.set_async(to_device(torch, one), 3, MAX)
            got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
            counts = texel_counts(one, W, H)
            assert_exact(got, counts, sim.expected_frame(oracle, counts))
            assert smap.debug_blocks().tolist() == [[13, 0, 2, 0]]
        _, blocks, _ = async_parity(lib, renderer, torch, oracle, W, H, TABLE_64x40, unit=3, set_scene=False)
        assert len(blocks) == 203
        async_parity(lib, renderer, torch, oracle, 44, 27, EXAMPLE, unit=1, accel=BRUTE, set_scene=False)
    finally:
        renderer.tune(refill_reserve=None)


@pytest.mark.gpu
def test_device_built_scene(lib, renderer, torch, oracle):
    """1 160 spheres: the device build with its L2 grid / treelet walks."""
    async_parity(lib, renderer, torch, oracle, 44, 27, EXAMPLE, unit=5, k=17)
    assert renderer.scene_array(8)["device_built"]


@pytest.mark.gpu
def test_rows_map_and_sample_base(lib, renderer, torch, oracle):
    async_parity(lib, renderer, torch, oracle, 44, len(ROWS), EXAMPLE[:18], unit=5, rows=ROWS, base=1000, image=(44, 40))


@pytest.mark.gpu
def test_queued_back_to_back(lib, renderer, torch, oracle):
    """Set calls and frames alternate on one map without a wait in between: every frame renders the
    table set before it (the planner runs behind the frames queued on the map, the frames behind the
    planner); a synchronous set call and a plain frame afterwards find everything as they left it."""
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    pa, po = plain_exact(lib, renderer, torch, oracle, W, H, 6)
    tables = [TABLE_64x40, TABLE_64x40[::-1], [6] * 40, [0] * 40, TABLE_64x40]
    with renderer.sample_map(W, H) as smap:
        frames = []
        for i, table in enumerate(tables):
            smap.set_async(to_device(torch, table), (3, 0, 128, 1, 5)[i], MAX)
            frames.append(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
            frames.append(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        torch.cuda.synchronize()
        for i, bufs in enumerate(frames):
            counts = texel_counts(tables[i // 2], W, H)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts))
        acc, out, _ = to_host(frames[4])
        assert np.array_equal(acc, pa) and np.array_equal(out, po)   # the uniform map is the plain frame
        check_plan(lib, smap, tables[-1], 5, MAX)
        # host-planned again, under either schedule; then device-planned again
        for schedule in (ONE, 0):
            smap.schedule(schedule)
            info = set_map(torch, smap, EXAMPLE + [3] * 16)
            assert info.max_count == 64 and smap.info.levels == info.levels > 0
            counts = texel_counts(EXAMPLE + [3] * 16, W, H)
            assert_exact(to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H)), counts,
                         sim.expected_frame(oracle, counts))
        smap.set_async(to_device(torch, tables[1]), 3, MAX)
        counts = texel_counts(tables[1], W, H)
        assert_exact(to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H)), counts,
                     sim.expected_frame(oracle, counts))
        check_plan(lib, smap, tables[1], 3, MAX)
    qa, qo = plain_exact(lib, renderer, torch, oracle, W, H, 6)
    assert np.array_equal(pa, qa) and np.array_equal(po, qo)


@pytest.mark.gpu
def test_refusals(lib, renderer, torch, oracle):
    from rtvk import RtError
    W, H = 44, 27
    renderer.set_scene(sim.scene(oracle))
    acc, out, cnt = sentinels(torch, W, H)

    def refused(field, call):
        with pytest.raises(RtError) as e:
            call()
        assert e.value.code == -1 and field in str(e.value), str(e.value)

    with renderer.sample_map(W, H) as smap:
        dev = to_device(torch, EXAMPLE)
        smap.schedule(ONE, 3)
        set_map(torch, smap, EXAMPLE)
        held = smap.schedule_info()
        refused("count_cap", lambda: smap.set_async(dev, 0, (1 << 19) + 1))
        refused("unit_samples", lambda: smap.set_async(dev, (1 << 19) + 1, 64))
        assert lib.load_library().rt_sample_map_set_device_async(None, dev.data_ptr(), 0, 64, None) == -1
        assert smap.schedule_info() == held and smap.info.levels == 10   # the refusals left the map as it was
        smap.set_async(dev, 3, 128)
        # the frame's cap is checked against count_cap: the host knows no more of the map
        refused("count_cap 128", lambda: renderer.render_sample_map(rci_of(lib, oracle, 64, W, H), acc, out, smap,
                                                                    sample_count=cnt, options=lib.make_options(rng_mode=HASH)))
        torch.cuda.synchronize()
        assert float((acc + 1.0).abs().sum()) == 0.0 and int((out != 7).sum()) == 0 and int((cnt != -1).sum()) == 0
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H, cap=128))
        counts = texel_counts(EXAMPLE, W, H)
        assert_exact(got, counts, sim.expected_frame(oracle, counts))
        check_plan(lib, smap, EXAMPLE, 3, 128)
