"""Sample-map frames (rt_render_sample_map_device) on the GPU: every texel of a
frame rendered with n[t] samples on tile t against the unchanged oracle.

A tile that holds n samples of the counter-based stream is the uniform n-spp frame bit for bit, so
adaptive_sim.expected_frame(oracle, counts) is the exact reference of any count map: accumulator,
rgba8 and the per-texel counts are compared in every texel, with the output buffers pre-filled with
sentinels. The shapes are the smallest at which the code can go wrong: bands ragged in both axes,
prefix lengths that are no multiple of anything, one and many levels, zero counts.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402

HASH = 2
BRUTE, AUTO = 1, 0
MIN, STEP, MAX, THR = 8, 8, 64, 0.2   # the adaptive tests' setting
# DESIGN.md §3.1.2's worked example (44x27: 6 x 4 tiles): zeros, odd counts, 1, repeats, the cap 64
EXAMPLE = [0, 1, 2, 7, 8, 64, 64, 3, 0, 0, 5, 12, 12, 1, 2, 2, 9, 9, 9, 30, 0, 64, 7, 8]
# the same style for 64x40 (8 x 5 tiles)
TABLE_64x40 = EXAMPLE + [64, 0, 1, 33, 17, 17, 2, 5, 64, 11, 3, 0, 7, 7, 21, 1]
ROWS = np.array([37, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19, 24, 25, 31, 32, 33, 39], np.int32)   # of a 44x40 image


def table_for(W, H):
    return {(44, 27): EXAMPLE, (64, 40): TABLE_64x40}[(W, H)]


def texel_counts(table, W, H):
    """The per-texel count map [H, W] of a tile table."""
    t = np.asarray(table, np.uint32).reshape((H + 7) // 8, (W + 7) // 8)
    return np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:H, :W].copy()


@pytest.fixture(scope="module")
def lib(oracle):
    import rtvk
    return rtvk


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def renderer(lib, torch):
    r = lib.Renderer(0)
    yield r
    r.close()


def rci_of(lib, oracle, spp, W, H):
    return lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())


def sentinels(torch, W, H):
    return (torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda"),
            torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda"),
            torch.full((H, W), -1, dtype=torch.int32, device="cuda"))


def to_host(bufs):
    acc, out, cnt = bufs
    return acc.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)


def set_map(torch, smap, table, quantum=0):
    return smap.set(torch.from_numpy(np.asarray(table, np.int32)).cuda(), quantum)


def frame_options(lib, accel=AUTO, base=0, options=None):
    """rt_options of a map, feedback or adaptive frame: the hash stream from sample `base`, with `accel`;
    or, given ready-made `options`, a copy of them (their accel and reserved words) with that stream
    and base."""
    if options is None:
        return lib.make_options(rng_mode=HASH, accel=accel, sample_base=base)
    o = type(options).from_buffer_copy(options)
    o.rng_mode, o.sample_base = HASH, base
    return o


def queue_map_frame(lib, renderer, torch, oracle, smap, W, H, accel=AUTO, rows=None, base=0, image=None, cap=MAX,
                    options=None):
    """Queues one frame of `smap` into fresh sentinel buffers; no synchronisation."""
    iw, ih = image if image else (W, H)
    bufs = sentinels(torch, W, H)
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    renderer.render_sample_map(rci_of(lib, oracle, cap, iw, ih), bufs[0], bufs[1], smap, sample_count=bufs[2],
                               rows=rows_t, options=frame_options(lib, accel, base, options))
    return bufs


def assert_exact(got, counts, ref):
    acc, out, cnt = got
    np.testing.assert_array_equal(cnt, counts)
    bad = np.argwhere(acc != ref[0])
    assert bad.size == 0, f"{len(bad)} accumulator floats differ, first at {bad[:4].tolist()}"
    np.testing.assert_array_equal(out, ref[1])


def map_parity(lib, renderer, torch, oracle, W, H, table, quantum=0, k=11, set_scene=True, **kw):
    """One map frame of `table` against the oracle at the (quantised) counts. Returns the set call's info.
    `k`: the scene's key in adaptive_sim; `options` (in kw): ready-made rt_options, see frame_options."""
    if set_scene:
        renderer.set_scene(sim.scene(oracle, k))
    q = max(1, quantum)
    quantised = (np.asarray(table, np.int64) + q - 1) // q * q
    counts = texel_counts(quantised, W, H)
    sk = {key: kw[key] for key in ("rows", "base", "image") if key in kw}
    ref = sim.expected_frame(oracle, counts, k=k, **sk)
    with renderer.sample_map(W, H) as smap:
        info = set_map(torch, smap, table, quantum)
        bufs = queue_map_frame(lib, renderer, torch, oracle, smap, W, H, **kw)
        torch.cuda.synchronize()
        assert_exact(to_host(bufs), counts, ref)
    assert info.samples == int(counts.astype(np.int64).sum()) and info.tiles == len(table)
    return info


def adaptive_parity(lib, renderer, torch, oracle, W, H, k=11, thr=THR, options=None):
    """An adaptive frame of the existing kind against the simulation and the oracle (`k`: the scene's
    key in adaptive_sim, the renderer's current scene; `options`: see frame_options)."""
    counts, info_sim = sim.simulate(sim.cube(oracle, W, H, MAX, k=k), MIN, STEP, MAX, lib.threshold_q16(thr))
    sim.assert_not_vacuous(counts, MAX)
    bufs = sentinels(torch, W, H)
    info = renderer.render_adaptive(rci_of(lib, oracle, MAX, W, H), bufs[0], bufs[1], sample_count=bufs[2],
                                    options=frame_options(lib, options=options), adaptive=lib.make_adaptive(thr, MIN, STEP))
    torch.cuda.synchronize()
    got = to_host(bufs)
    assert_exact(got, counts, sim.expected_frame(oracle, counts, k=k))
    assert (info.passes, info.samples, info.tiles_capped) == (info_sim["passes"], info_sim["samples"],
                                                              info_sim["tiles_capped"])
    return counts, got, info


def plain_exact(lib, renderer, torch, oracle, W, H, spp):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    renderer.render_device(rci_of(lib, oracle, spp, W, H), acc, out, options=lib.make_options(rng_mode=HASH))
    torch.cuda.synchronize()
    ra, ro, _ = oracle.render(sim.scene(oracle), oracle.render_call_info(spp, W, H), W, H,
                              opts=oracle.options(rng_mode=HASH))
    assert np.array_equal(acc.cpu().numpy(), ra) and np.array_equal(out.cpu().numpy(), ro)
    return acc.cpu().numpy(), out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [BRUTE, AUTO])
@pytest.mark.parametrize("shape", [(64, 40), (44, 27)])
def test_parity(lib, renderer, torch, oracle, shape, accel):
    info = map_parity(lib, renderer, torch, oracle, *shape, table_for(*shape), accel=accel)
    assert (info.levels, info.min_count, info.max_count) == ((14, 1, 64) if shape == (64, 40) else (10, 1, 64))


@pytest.mark.gpu
def test_device_built_scene(lib, renderer, torch, oracle):
    """1 160 spheres: the device build with its L2 grid / treelet walks."""
    map_parity(lib, renderer, torch, oracle, 44, 27, EXAMPLE, k=17)
    assert renderer.scene_array(8)["device_built"]


@pytest.mark.gpu
def test_many_tiles_few_levels(lib, renderer, torch, oracle):
    """200x120: 375 tiles in 5 levels, prefix lengths that are no multiple of anything."""
    table = np.random.default_rng(375).choice([0, 1, 2, 3, 5, 6], 375)
    plan = lib.sample_map_plan(table)
    assert plan["levels"].tolist() == [1, 2, 3, 5, 6] and all(c % 8 for c in plan["level_tiles"].tolist())
    info = map_parity(lib, renderer, torch, oracle, 200, 120, table, cap=6)
    assert info.levels == 5 and info.tile_launches == int(plan["level_tiles"].sum())


@pytest.mark.gpu
def test_uniform_and_zero_maps(lib, renderer, torch, oracle):
    W, H = 44, 27
    renderer.set_scene(sim.scene(oracle))
    pa, po = plain_exact(lib, renderer, torch, oracle, W, H, 6)
    with renderer.sample_map(W, H) as smap:
        info = set_map(torch, smap, [6] * 24)
        assert (info.levels, info.tile_launches, info.samples) == (1, 24, 6 * W * H)
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert np.array_equal(acc, pa) and np.array_equal(out, po) and (cnt == 6).all()
        info = set_map(torch, smap, [0] * 24)
        assert (info.levels, info.tile_launches, info.samples, info.min_count, info.max_count) == (0, 0, 0, 0, 0)
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
    # the 0-sample frame, as oracle.render(spp=0) gives it
    ra, ro = sim.expected_frame(oracle, np.zeros((H, W), np.uint32))
    assert np.array_equal(acc, ra) and np.array_equal(out, ro) and (cnt == 0).all()
    assert (acc == np.array([0, 0, 0, 1], np.float32)).all() and (out == np.array([0, 0, 0, 255], np.uint8)).all()


@pytest.mark.gpu
def test_replay_of_an_adaptive_frame(lib, renderer, torch, oracle):
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    counts, (acc_a, out_a, cnt_a), info_a = adaptive_parity(lib, renderer, torch, oracle, W, H)
    with renderer.sample_map(W, H) as smap:
        info = smap.set_from_adaptive(0)
        assert info.samples == info_a.samples and info.tiles == info_a.tiles == 40
        assert (info.min_count, info.max_count) == (int(counts.min()), int(counts.max()))
        np.testing.assert_array_equal(smap.debug_plan()["quantised"], counts[::8, ::8].ravel())
        acc, out, cnt = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert np.array_equal(acc, acc_a) and np.array_equal(out, out_a) and np.array_equal(cnt, cnt_a)
        # quantum 16: the rounded-up counts, and the oracle's frame at them
        info = smap.set_from_adaptive(16)
        up = (counts.astype(np.int64) + 15) // 16 * 16
        assert info.samples == int(up.sum()) and info.levels == len(np.unique(up))
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        assert_exact(got, up.astype(np.uint32), sim.expected_frame(oracle, up.astype(np.uint32)))


@pytest.mark.gpu
def test_rows_map_and_sample_base(lib, renderer, torch, oracle):
    """Non-contiguous rows of a 44x40 image (the adaptive tests' rows) and sample_base = 1000."""
    map_parity(lib, renderer, torch, oracle, 44, len(ROWS), EXAMPLE[:18], rows=ROWS, base=1000, image=(44, 40))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 7])
def test_order_and_chunk_independence(lib, renderer, torch, oracle, chunks):
    renderer.tune(sample_chunks=chunks)
    try:
        map_parity(lib, renderer, torch, oracle, 64, 40, TABLE_64x40)
    finally:
        renderer.tune(sample_chunks=None)


@pytest.mark.gpu
def test_back_to_back_frames(lib, renderer, torch, oracle):
    """Two frames of different maps into different buffers on one stream, one synchronisation; then an
    adaptive and a plain frame are still exact: the planes are left zero, no tile state is stale."""
    W, H = 64, 40
    renderer.set_scene(sim.scene(oracle))
    other = TABLE_64x40[::-1]
    with renderer.sample_map(W, H) as m1, renderer.sample_map(W, H) as m2:
        set_map(torch, m1, TABLE_64x40)
        set_map(torch, m2, other)
        b1 = queue_map_frame(lib, renderer, torch, oracle, m1, W, H)
        b2 = queue_map_frame(lib, renderer, torch, oracle, m2, W, H)
        b3 = queue_map_frame(lib, renderer, torch, oracle, m1, W, H)
        torch.cuda.synchronize()
        for bufs, table in ((b1, TABLE_64x40), (b2, other), (b3, TABLE_64x40)):
            counts = texel_counts(table, W, H)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts))
        adaptive_parity(lib, renderer, torch, oracle, W, H)
        plain_exact(lib, renderer, torch, oracle, W, H, 6)
        # and a map frame after them, on a smaller band of the same renderer
    map_parity(lib, renderer, torch, oracle, 44, 27, EXAMPLE, set_scene=False)


@pytest.mark.gpu
def test_debug_view_and_launch_records(lib, torch, oracle):
    W, H = 44, 27
    with lib.Renderer(0) as r:   # a fresh context: its launch ring starts empty
        r.set_scene(sim.scene(oracle))
        assert len(r.kernel_times()) == 0
        with r.sample_map(W, H) as smap:
            launches = 0
            for quantum, levels in ((0, 10), (16, 3), (0, 10)):
                info = set_map(torch, smap, EXAMPLE, quantum)
                want, got = lib.sample_map_plan(EXAMPLE, quantum), smap.debug_plan()
                for key in ("order", "levels", "level_tiles", "quantised"):
                    np.testing.assert_array_equal(got[key], want[key], err_msg=key)
                assert info.levels == levels == len(want["levels"])
                queue_map_frame(lib, r, torch, oracle, smap, W, H)
                torch.cuda.synchronize()
                launches += levels
                times = r.kernel_times()
                assert len(times) == launches and all(t > 0 for t in times)
                assert r.launch_ms(0) == times[-1]
            # rt_get_stats reports the last launch: samples [30, 64) on the 3 tiles of count 64 (tiles 5,
            # 6 and 21 with 32, 64 and 24 in-band pixels)
            assert r.stats().samples == 34 * (32 + 64 + 24)


@pytest.mark.gpu
def test_refusals(lib, renderer, torch, oracle):
    from rtvk import RtError, abi
    W, H = 44, 27
    with lib.Renderer(0) as fresh, fresh.sample_map(W, H) as smap:   # no scene yet
        set_map(torch, smap, EXAMPLE)
        bufs = sentinels(torch, W, H)
        with pytest.raises(RtError) as e:
            fresh.render_sample_map(rci_of(lib, oracle, MAX, W, H), bufs[0], bufs[1], smap,
                                    options=lib.make_options(rng_mode=HASH))
        assert e.value.code == -4   # RT_ERR_NO_SCENE
    renderer.set_scene(sim.scene(oracle))
    acc, out, cnt = sentinels(torch, W, H)

    def refused(field, smap, spp=MAX, r=renderer, bufs=(acc, out), **opt):
        o = dict(rng_mode=HASH)
        o.update(opt)
        with pytest.raises(RtError) as e:
            r.render_sample_map(rci_of(lib, oracle, spp, W, H), bufs[0], bufs[1], smap, options=lib.make_options(**o))
        assert e.value.code == -1 and field in str(e.value), str(e.value)   # RT_ERR_INVALID_ARGUMENT

    def set_refused(field, smap, table, quantum=0):
        with pytest.raises(RtError) as e:
            set_map(torch, smap, table, quantum)
        assert e.value.code == -1 and field in str(e.value), str(e.value)

    with renderer.sample_map(W, H) as smap, renderer.sample_map(64, 40) as big:
        refused("never set", smap)
        with pytest.raises(RtError) as e:
            smap.set_from_adaptive(0)    # no adaptive frame on this context since its buffers were made
        assert e.value.code == -1 and "adaptive frame" in str(e.value)
        set_map(torch, smap, EXAMPLE)
        set_map(torch, big, TABLE_64x40)
        refused("rng_mode", smap, rng_mode=abi.RT_RNG_PIXEL_STREAM)
        refused("rng_mode", smap, rng_mode=abi.RT_RNG_SAMPLE_COUNTER)
        refused("accumulate", smap, accumulate=True)
        refused("band size", big)                       # a 64x40 map for 44x27 buffers
        refused("samplesPerRenderCall", smap, spp=63)   # the cap below the map's max_count
        refused("2^19", smap, spp=(1 << 19) + 1)
        refused("sample_base", smap, sample_base=0xffffffff)
        with lib.Renderer(0) as other:
            other.set_scene(sim.scene(oracle))
            refused("another context", smap, r=other)
        # the set calls: a refusal names the tile or the level count and leaves the map as it was
        bad = list(EXAMPLE)
        bad[7] = (1 << 19) + 1
        set_refused("tile_counts[7]", smap, bad)
        bad[7] = (1 << 19) - 1
        set_refused("tile_counts[7]", smap, bad, quantum=3)
        wide = renderer.sample_map(8 * 66, 8)            # 66 tiles: room for 65 levels
        set_refused("65 levels", wide, list(range(66)))
        set_refused("quantum", wide, list(range(66)))
        assert set_map(torch, wide, list(range(66)), quantum=2).levels == 33
        wide.close()
        adaptive_parity(lib, renderer, torch, oracle, 64, 40)
        with pytest.raises(RtError) as e:
            smap.set_from_adaptive(0)                    # a 64x40 adaptive frame for a 44x27 map
        assert e.value.code == -1 and "band size" in str(e.value)
        torch.cuda.synchronize()
        assert float((acc + 1.0).abs().sum()) == 0.0     # nothing rendered
        # after the refusals the map still holds EXAMPLE and a frame of it is exact
        assert smap.info.levels == 10
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        counts = texel_counts(EXAMPLE, W, H)
        assert_exact(got, counts, sim.expected_frame(oracle, counts))
