"""Feedback frames (rt_render_sample_map_feedback_device) on the GPU: a map frame
that renders its counts as two halves, measures every tile's noise from their difference, chooses the
tile's next count by the feedback rule and re-plans the map on the device.

The reference is the CPU simulation on adaptive_sim.cube, the per-sample integers of the unchanged
oracle: for a tile of n samples, A = the sum of samples [0, n / 2), B = of [n / 2, n), E and S as in
the adaptive criterion, the next count by the rule restated on adaptive_sim.converged. Every frame is
compared in every texel with adaptive_sim.expected_frame at the counts it rendered, the next counts
and (E, S) word for word with the simulation, and after each frame the device's block table with the
host planner's of the two halves. Canonical scene, 44x27 (6 x 4 tiles, ragged both ways), the
starting map a checkerboard of 16 and 32 over the tiles, min 4, max 64, threshold 0.3: the first step
raises some tiles, lowers one and keeps others. Helpers are tests/test_sample_map.py's."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
from test_sample_map import (AUTO, BRUTE, HASH, MAX, ROWS, assert_exact, frame_options, lib, queue_map_frame, renderer,   # noqa: E402
                             rci_of, sentinels, set_map, texel_counts, to_host, torch)

__all__ = ["lib", "renderer", "torch"]
W, H = 44, 27
TX, TY = 6, 4
LO, HI, THR = 4, 64, 0.3
START = [32 if (t % TX + t // TX) % 2 else 16 for t in range(TX * TY)]


def rule(E, S, n, m, thr, lo, hi):
    if n == 0:
        return 0
    if not sim.converged(E, S, n, m, thr):
        return min(hi, 2 * n)
    if sim.converged(E, S, n, m, thr >> 1):
        return max(lo, (n // 2 + 1) & ~1)
    return n


def step(Q, table, thr, lo=LO, hi=HI):
    """One feedback frame on the cube: (next table, [(E, S)] per tile)."""
    _, h, w, _ = Q.shape
    tx = (w + 7) // 8
    nxt, es = [], []
    for t, n in enumerate(table):
        q = Q[:, (t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8, :]
        a, b = q[:n // 2].sum(axis=0), q[n // 2:n].sum(axis=0)
        E, S = int(np.abs(a - b).sum()), int((a + b).sum())
        es.append((E, S))
        nxt.append(rule(E, S, n, q.shape[1] * q.shape[2], thr, lo, hi))
    return nxt, es


def queue_feedback(lib, renderer, torch, oracle, smap, w, h, fb, cap=MAX, accel=AUTO, rows=None, base=0, image=None, err=None,
                   options=None):
    iw, ih = image if image else (w, h)
    bufs = sentinels(torch, w, h)
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    renderer.render_sample_map_feedback(rci_of(lib, oracle, cap, iw, ih), bufs[0], bufs[1], smap, fb, sample_count=bufs[2],
                                        rows=rows_t, options=frame_options(lib, accel, base, options), tile_error=err)
    return bufs


def check_halves_table(lib, smap, table, cap, unit=0):
    """The device's table after a feedback frame planned `table` (even counts): the host planner's of
    the halves over [0, h), then the same entries over [h, 2 h)."""
    half = np.asarray(table, np.int64) // 2
    u0 = unit or min(128, max(32, cap // 32))
    U = lib.sample_map_device_unit(half, cap // 2, u0, lib.sample_map_device_capacity(len(half), cap // 2, u0))
    a = lib.sample_map_block_plan(half, 0, U)["blocks"].astype(np.int64)
    b = a.copy()
    shift = half[a[:, 0]]
    b[:, 1] += shift
    b[:, 2] += shift
    got = smap.debug_blocks()
    np.testing.assert_array_equal(got, np.concatenate([a, b]))
    assert smap.schedule_info() == {"schedule": 1, "unit_samples": U, "n_blocks": 2 * len(a)}
    np.testing.assert_array_equal(smap.debug_plan()["quantised"], table)


def chain(lib, renderer, torch, oracle, frames, thr=THR, lo=LO, hi=HI, start=START, w=W, h=H, k=11, cap=MAX, unit=0,
          async_start=False, with_error=True, set_scene=True, **kw):
    """`frames` feedback frames from `start`, each against the simulation. Returns the tables: [start,
    after frame 1, ...]. `k`: the scene's key in adaptive_sim (set_scene=False: it is the renderer's
    scene already); `options` (in kw): ready-made rt_options, see test_sample_map.frame_options."""
    if set_scene:
        renderer.set_scene(sim.scene(oracle, k))
    sk = {key: kw[key] for key in ("rows", "base", "image") if key in kw}
    Q = sim.cube(oracle, w, h, hi, k=k, **sk)
    fb = lib.make_feedback(thr, lo, hi, unit)
    thr_q = lib.threshold_q16(thr)
    tables = [list(start)]
    with renderer.sample_map(w, h) as smap:
        if async_start:
            smap.set_async(torch.from_numpy(np.asarray(start, np.int32)).cuda(), 0, cap)
        else:
            set_map(torch, smap, start)
        for _ in range(frames):
            table = tables[-1]
            nxt, es = step(Q, table, thr_q, lo, hi)
            err = torch.full((len(table), 2), -1, dtype=torch.int64, device="cuda") if with_error else None
            bufs = queue_feedback(lib, renderer, torch, oracle, smap, w, h, fb, cap=cap, err=err, **kw)
            torch.cuda.synchronize()
            counts = texel_counts(table, w, h)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts, k=k, **sk))
            assert smap.debug_feedback()["next"].tolist() == nxt
            if with_error:
                assert err.cpu().numpy().tolist() == [list(x) for x in es]
            check_halves_table(lib, smap, nxt, cap, unit)
            tables.append(nxt)
        moved = smap.debug_feedback()
        assert moved["raised"] == sum(sum(y > x for x, y in zip(a, b)) for a, b in zip(tables, tables[1:]))
        assert moved["lowered"] == sum(sum(y < x for x, y in zip(a, b)) for a, b in zip(tables, tables[1:]))
    return tables


def hist(table):
    return {int(n): int(c) for n, c in zip(*np.unique(table, return_counts=True))}


@pytest.mark.gpu
def test_first_frame_and_chain_to_the_fixed_point(lib, renderer, torch, oracle):
    tables = chain(lib, renderer, torch, oracle, 5)
    up = sum(b > a for a, b in zip(tables[0], tables[1]))
    down = sum(b < a for a, b in zip(tables[0], tables[1]))
    assert (up, down, len(START) - up - down) == (11, 1, 12)    # the first step: raised, lowered, kept
    assert up >= 1 and down >= 1 and up + down < len(START)
    assert hist(tables[4]) == {8: 1, 16: 3, 32: 18, 64: 2}     # four frames reach the fixed point ...
    assert tables[5] == tables[4]                               # ... and it is one


@pytest.mark.gpu
def test_threshold_anchors(lib, renderer, torch, oracle):
    tables = chain(lib, renderer, torch, oracle, 2, thr=0.0, with_error=False)
    assert set(tables[2]) == {64}                               # nothing converges: 16 -> 32 -> 64
    tables = chain(lib, renderer, torch, oracle, 3, thr=16.0, with_error=False)
    assert set(tables[3]) == {4}                                # everything does: 32 -> 16 -> 8 -> 4


@pytest.mark.gpu
def test_rows_map_and_sample_base(lib, renderer, torch, oracle):
    start = [32 if (t % TX + t // TX) % 2 else 16 for t in range(18)]
    tables = chain(lib, renderer, torch, oracle, 2, start=start, h=len(ROWS), rows=ROWS, base=1000, image=(44, 40), unit=5)
    assert tables[1] != tables[0]


@pytest.mark.gpu
def test_brute_force_and_async_start(lib, renderer, torch, oracle):
    """accel brute; the starting map set by set_async (odd counts there are rounded up to even)."""
    tables = chain(lib, renderer, torch, oracle, 2, accel=BRUTE, async_start=True, unit=3)
    assert tables[1] != tables[0]
    odd = [c - 1 if t % 3 == 0 else c for t, c in enumerate(START)]
    renderer.set_scene(sim.scene(oracle))
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, odd)
        got = to_host(queue_feedback(lib, renderer, torch, oracle, smap, W, H, lib.make_feedback(THR, LO, HI)))
        counts = texel_counts(START, W, H)                      # 15 -> 16, 31 -> 32
        assert_exact(got, counts, sim.expected_frame(oracle, counts))


@pytest.mark.gpu
def test_device_built_scene(lib, renderer, torch, oracle):
    """1 160 spheres (k = 17), a ladder of 4 .. 16."""
    start = [8 if (t % TX + t // TX) % 2 else 4 for t in range(TX * TY)]
    chain(lib, renderer, torch, oracle, 2, lo=2, hi=16, start=start, k=17, cap=16, thr=0.3)
    assert renderer.scene_array(8)["device_built"]


@pytest.mark.gpu
def test_plain_frame_of_a_halves_planned_map(lib, renderer, torch, oracle):
    """rt_render_sample_map_device on the map a feedback frame left: one launch over both halves, the
    image of the next counts; and a feedback frame after it renders the same image."""
    renderer.set_scene(sim.scene(oracle))
    nxt, _ = step(sim.cube(oracle, W, H, HI), START, lib.threshold_q16(THR))
    counts = texel_counts(nxt, W, H)
    ref = sim.expected_frame(oracle, counts)
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, START)
        fb = lib.make_feedback(THR, LO, HI)
        queue_feedback(lib, renderer, torch, oracle, smap, W, H, fb)
        launches = len(renderer.kernel_times())
        plain = queue_map_frame(lib, renderer, torch, oracle, smap, W, H)
        again = queue_feedback(lib, renderer, torch, oracle, smap, W, H, fb)
        torch.cuda.synchronize()
        assert_exact(to_host(plain), counts, ref)
        assert_exact(to_host(again), counts, ref)
        nxt2, _ = step(sim.cube(oracle, W, H, HI), nxt, lib.threshold_q16(THR))   # what the second frame planned
        assert smap.info.samples == int(texel_counts(nxt2, W, H).astype(np.int64).sum())
        assert len(renderer.kernel_times()) == min(64, launches + 3)   # one launch, then two


@pytest.mark.gpu
def test_no_host_wait(lib, torch, oracle):
    """Four frames queued back to back before the first synchronize; no host wait inside the calls."""
    fb = lib.make_feedback(THR, LO, HI)
    Q = sim.cube(oracle, W, H, HI)
    thr_q = lib.threshold_q16(THR)
    with lib.Renderer(0) as r:
        r.set_scene(sim.scene(oracle))
        with r.sample_map(W, H) as smap:
            set_map(torch, smap, START)
            frames = [queue_feedback(lib, r, torch, oracle, smap, W, H, fb) for _ in range(4)]
            assert r.host_waits() == 0
            torch.cuda.synchronize()
            table = START
            for bufs in frames:
                counts = texel_counts(table, W, H)
                assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts))
                table, _ = step(Q, table, thr_q)
            assert smap.debug_feedback()["next"].tolist() == table
            assert r.host_waits() == 0


@pytest.mark.gpu
def test_refusals(lib, renderer, torch, oracle):
    from rtvk import RtError, abi
    renderer.set_scene(sim.scene(oracle))
    acc, out, cnt = sentinels(torch, W, H)

    def refused(field, fb=None, spp=MAX, m=None, r=renderer, **opt):
        o = dict(rng_mode=HASH)
        o.update(opt)
        with pytest.raises(RtError) as e:
            r.render_sample_map_feedback(rci_of(lib, oracle, spp, W, H), acc, out, m if m is not None else smap,
                                         fb if fb is not None else lib.make_feedback(THR, LO, HI), sample_count=cnt,
                                         options=lib.make_options(**o))
        assert e.value.code == -1 and field in str(e.value), str(e.value)

    with renderer.sample_map(W, H) as smap, renderer.sample_map(8, 8) as small:
        refused("never set")
        set_map(torch, smap, START)
        set_map(torch, small, [16])
        held = smap.info
        # the checks shared with rt_render_sample_map_device (tests/test_sample_map.py::test_refusals)
        refused("band size", m=small)                     # an 8x8 map for 44x27 buffers
        refused("sample_base", sample_base=0xffffffff)
        with lib.Renderer(0) as other:
            other.set_scene(sim.scene(oracle))
            refused("another context", r=other)
        refused("rng_mode", rng_mode=abi.RT_RNG_PIXEL_STREAM)
        refused("accumulate", accumulate=True)
        refused("must be even", spp=65)
        refused("max_count", fb=lib.make_feedback(THR, LO, 16), spp=30)   # the cap below what the map holds
        refused("max_spp", fb=lib.make_feedback(THR, LO, 128))          # the cap below max_spp
        refused("threshold", fb=lib.make_feedback(float("nan"), LO, HI))
        refused("threshold", fb=lib.make_feedback(16.5, LO, HI))
        refused("threshold", fb=lib.make_feedback(-0.1, LO, HI))
        refused("min_spp", fb=lib.make_feedback(THR, 3, HI))
        refused("min_spp", fb=lib.make_feedback(THR, 0, HI))
        refused("min_spp", fb=lib.make_feedback(THR, 4, 63))
        refused("min_spp", fb=lib.make_feedback(THR, 66, 64))
        refused("unit_samples", fb=lib.make_feedback(THR, LO, HI, (1 << 19) + 1))
        torch.cuda.synchronize()
        assert float((acc + 1.0).abs().sum()) == 0.0 and int((out != 7).sum()) == 0 and int((cnt != -1).sum()) == 0
        assert smap.info.samples == held.samples and smap.info.levels == held.levels   # the map is as it was
        got = to_host(queue_map_frame(lib, renderer, torch, oracle, smap, W, H))
        counts = texel_counts(START, W, H)
        assert_exact(got, counts, sim.expected_frame(oracle, counts))
