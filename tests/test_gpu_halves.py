"""The hand-over of the two halves on the GPU (rt_render_adaptive_halves_device,
rt_render_sample_map_feedback_halves_device): accum_a, accum_b and half_count of a
feedback and of an adaptive frame against the CPU model (tests/halves_sim.py) in every texel, bit for
bit, and against oracle.render at the half's sample range; everything the plain calls write against
what their own tests expect (test_sample_map_feedback.py's chain, test_adaptive.py's parity).
Canonical scene, 44x27: 6 x 4 tiles, ragged both ways. Every output starts as sentinels, so a texel
the resolve skipped shows. Helpers are those of the two plain test files."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
import halves_sim as hs      # noqa: E402
import test_adaptive as ta   # noqa: E402
from test_sample_map import (HASH, MAX, ROWS, adaptive_parity, assert_exact, lib, map_parity, plain_exact, renderer,   # noqa: E402
                             rci_of, sentinels, set_map, table_for, texel_counts, to_host, torch)
from test_sample_map_feedback import H, HI, LO, START, THR, TX, W, check_halves_table, step   # noqa: E402

__all__ = ["lib", "renderer", "torch"]
ZERO_TILE, ODD_TILE, ODD = 5, 10, 7


def edited(start):
    """The checkerboard of 16 and 32 with one tile of count 0 and one of an odd count."""
    s = list(start)
    s[ZERO_TILE], s[ODD_TILE] = 0, ODD
    return s


def half_sentinels(torch, w, h):
    return (torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda"),
            torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda"),
            torch.full((h, w), -1, dtype=torch.int32, device="cuda"))


def halves_to_host(hb):
    return hb[0].cpu().numpy(), hb[1].cpu().numpy(), hb[2].cpu().numpy().astype(np.uint32)


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[:4].tolist()}"


def assert_halves(got, want):
    assert_bits(got[0], want[0], "accum_a")
    assert_bits(got[1], want[1], "accum_b")
    np.testing.assert_array_equal(got[2], want[2])


def oracle_halves(oracle, half, base=0, rows=None, image=None, k=11):
    """(accum_a, accum_b) from the oracle: a texel of half count h holds oracle.render at (h, base) and
    at (h, base + h)."""
    hh, ww = half.shape
    iw, ih = image if image else (ww, hh)
    rt = None if rows is None else tuple(int(r) for r in rows)
    a = np.zeros((hh, ww, 4), np.float32)
    b = np.zeros((hh, ww, 4), np.float32)
    for h in np.unique(half):
        sel = half == h
        a[sel] = sim._uniform(oracle, k, ww, hh, iw, ih, rt, base, int(h))[0][sel]
        b[sel] = sim._uniform(oracle, k, ww, hh, iw, ih, rt, base + int(h), int(h))[0][sel]
    return a, b


def simulated_tables(Q, start, frames, thr_q):
    """[the table frame 0 renders (start rounded up to even), what it plans, ...] and (E, S) per frame."""
    tables, errors = [hs.even_table(start)], []
    for _ in range(frames):
        nxt, es = step(Q, tables[-1], thr_q, LO, HI)
        tables.append(nxt)
        errors.append(es)
    return tables, errors


def assert_feedback_not_vacuous(start, tables, frames):
    assert start[ZERO_TILE] == 0 and start[ODD_TILE] % 2 == 1 and tables[0][ODD_TILE] == start[ODD_TILE] + 1
    for table in tables[:frames]:   # every table a frame renders
        assert table[ZERO_TILE] == 0
        assert len({n for n in table if n}) >= 3, table


def queue_feedback_halves(lib, renderer, torch, oracle, smap, w, h, fb, rows=None, base=0, image=None, err=None):
    iw, ih = image if image else (w, h)
    bufs, hb = sentinels(torch, w, h), half_sentinels(torch, w, h)
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    renderer.render_sample_map_feedback(rci_of(lib, oracle, MAX, iw, ih), bufs[0], bufs[1], smap, fb, sample_count=bufs[2],
                                        rows=rows_t, options=lib.make_options(rng_mode=HASH, sample_base=base),
                                        tile_error=err, accum_a=hb[0], accum_b=hb[1], half_count=hb[2])
    return bufs, hb


def feedback_chain(lib, renderer, torch, oracle, start, frames, w=W, h=H, **kw):
    renderer.set_scene(sim.scene(oracle))
    Q = sim.cube(oracle, w, h, HI, **kw)
    thr_q = lib.threshold_q16(THR)
    tables, errors = simulated_tables(Q, start, frames, thr_q)
    assert_feedback_not_vacuous(start, tables, frames)   # on the simulation, before the GPU is touched
    fb = lib.make_feedback(THR, LO, HI)
    with renderer.sample_map(w, h) as smap:
        set_map(torch, smap, start)
        for f in range(frames):
            table = tables[f]
            err = torch.full((len(table), 2), -1, dtype=torch.int64, device="cuda")
            bufs, hb = queue_feedback_halves(lib, renderer, torch, oracle, smap, w, h, fb, err=err, **kw)
            torch.cuda.synchronize()
            got = halves_to_host(hb)
            want = hs.feedback_halves(Q, table)
            assert_halves(got, want)
            oa, ob = oracle_halves(oracle, want[2], **kw)
            assert_bits(got[0], oa, "accum_a against the oracle")
            assert_bits(got[1], ob, "accum_b against the oracle")
            assert np.all(got[0][texel_counts(table, w, h) == 0] == np.float32([0, 0, 0, 1]))
            # what the plain call writes, as test_sample_map_feedback.chain expects it
            counts = texel_counts(table, w, h)
            assert_exact(to_host(bufs), counts, sim.expected_frame(oracle, counts, **kw))
            assert smap.debug_feedback()["next"].tolist() == tables[f + 1]
            assert err.cpu().numpy().tolist() == [list(x) for x in errors[f]]
            check_halves_table(lib, smap, tables[f + 1], MAX)
    return tables


@pytest.mark.gpu
def test_feedback_halves_three_frames(lib, renderer, torch, oracle):
    tables = feedback_chain(lib, renderer, torch, oracle, edited(START), 3)
    assert tables[1] != tables[0]


@pytest.mark.gpu
def test_feedback_halves_rows_map_and_sample_base(lib, renderer, torch, oracle):
    start = edited([32 if (t % TX + t // TX) % 2 else 16 for t in range(18)])
    feedback_chain(lib, renderer, torch, oracle, start, 3, h=len(ROWS), rows=ROWS, base=1000, image=(44, 40))


def gpu_adaptive_halves(lib, renderer, torch, oracle, w, h, thr=ta.THR, base=0):
    bufs, hb = sentinels(torch, w, h), half_sentinels(torch, w, h)
    info = renderer.render_adaptive(rci_of(lib, oracle, ta.MAX, w, h), bufs[0], bufs[1], sample_count=bufs[2],
                                    options=lib.make_options(rng_mode=HASH, sample_base=base),
                                    adaptive=lib.make_adaptive(thr, ta.MIN, ta.STEP), accum_a=hb[0], accum_b=hb[1],
                                    half_count=hb[2])
    torch.cuda.synchronize()
    return to_host(bufs) + (info,), halves_to_host(hb)


@pytest.mark.gpu
def test_adaptive_halves(lib, renderer, torch, oracle):
    renderer.set_scene(sim.scene(oracle))
    Q = sim.cube(oracle, W, H, ta.MAX)
    thr_q = lib.threshold_q16(ta.THR)
    counts, info_sim = sim.simulate(Q, ta.MIN, ta.STEP, ta.MAX, thr_q)
    sim.assert_not_vacuous(counts, ta.MAX)
    assert len(sim.histogram(counts)) == 7
    want = hs.adaptive_halves(Q, ta.MIN, ta.STEP, ta.MAX, thr_q)
    np.testing.assert_array_equal(want[3], counts)
    got, halves = gpu_adaptive_halves(lib, renderer, torch, oracle, W, H)
    assert_halves(halves, want[:3])
    ta.assert_frame(got, counts, info_sim, sim.expected_frame(oracle, counts))   # test_adaptive.parity's expectations


@pytest.mark.gpu
@pytest.mark.parametrize("base", [0, 1000])
def test_adaptive_halves_threshold_sixteen(lib, renderer, torch, oracle, base):
    """One pass: A is the uniform frame of min / 2 samples at b, B the one at b + min / 2."""
    renderer.set_scene(sim.scene(oracle))
    got, halves = gpu_adaptive_halves(lib, renderer, torch, oracle, W, H, thr=16.0, base=base)
    half = np.full((H, W), ta.MIN // 2, np.uint32)
    oa, ob = oracle_halves(oracle, half, base=base)
    assert_halves(halves, (oa, ob, half))
    assert (got[2] == ta.MIN).all() and got[3].passes == 1


@pytest.mark.gpu
def test_half_count_is_optional(lib, renderer, torch, oracle):
    renderer.set_scene(sim.scene(oracle))
    Q = sim.cube(oracle, W, H, HI)
    table = hs.even_table(edited(START))
    want = hs.feedback_halves(Q, table)
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, table)
        bufs, hb = sentinels(torch, W, H), half_sentinels(torch, W, H)
        renderer.render_sample_map_feedback(rci_of(lib, oracle, MAX, W, H), bufs[0], bufs[1], smap,
                                            lib.make_feedback(THR, LO, HI), options=lib.make_options(rng_mode=HASH),
                                            accum_a=hb[0], accum_b=hb[1])
        torch.cuda.synchronize()
    assert_bits(hb[0].cpu().numpy(), want[0], "accum_a")
    assert_bits(hb[1].cpu().numpy(), want[1], "accum_b")
    assert int((hb[2] != -1).sum()) == 0 and int((bufs[2] != -1).sum()) == 0   # neither count plane was given


@pytest.mark.gpu
def test_planes_are_left_zero(lib, renderer, torch, oracle):
    """After a halves frame of each kind, a plain map frame, a plain adaptive frame and a plain render
    on the same context are exact: the resolve zeroed both plane sets."""
    renderer.set_scene(sim.scene(oracle))
    fb = lib.make_feedback(THR, LO, HI)

    def plain_frames():
        map_parity(lib, renderer, torch, oracle, W, H, table_for(W, H), set_scene=False)
        adaptive_parity(lib, renderer, torch, oracle, W, H)
        plain_exact(lib, renderer, torch, oracle, W, H, 5)

    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, edited(START))
        queue_feedback_halves(lib, renderer, torch, oracle, smap, W, H, fb)
        plain_frames()
    gpu_adaptive_halves(lib, renderer, torch, oracle, W, H)
    plain_frames()


@pytest.mark.gpu
def test_the_resolve_alone_on_zero_planes(lib, renderer, torch, oracle):
    """rt_debug_adaptive_resolve, the timing entry point: zero planes resolve to (0, 0, 0, 1), black
    bytes and the given count in every texel, in both forms, and leave the context as a frame does."""
    renderer.set_scene(sim.scene(oracle))
    for with_halves in (False, True):
        bufs, hb = sentinels(torch, W, H), half_sentinels(torch, W, H)
        kw = dict(accum_a=hb[0], accum_b=hb[1], half_count=hb[2]) if with_halves else {}
        renderer.adaptive_resolve(bufs[0], bufs[1], 6, sample_count=bufs[2], **kw)
        torch.cuda.synchronize()
        acc, out, cnt = to_host(bufs)
        assert np.all(acc == np.float32([0, 0, 0, 1])) and np.all(out == np.uint8([0, 0, 0, 255])) and np.all(cnt == 6)
        a, b, half = halves_to_host(hb)
        if with_halves:
            assert np.all(a == np.float32([0, 0, 0, 1])) and np.all(b == np.float32([0, 0, 0, 1])) and np.all(half == 3)
        else:
            assert np.all(a == -1.0) and np.all(b == -1.0) and np.all(hb[2].cpu().numpy() == -1)
    with pytest.raises(lib.RtError, match="accum_a and accum_b"):
        renderer.adaptive_resolve(bufs[0], bufs[1], 6, accum_a=hb[0], accum_b=hb[0])
    adaptive_parity(lib, renderer, torch, oracle, W, H)
    plain_exact(lib, renderer, torch, oracle, W, H, 5)


@pytest.mark.gpu
def test_plain_entry_points_give_the_same_bytes(lib, renderer, torch, oracle):
    """The calls without halves on the same inputs: the bytes of the halves calls' shared outputs, which
    the tests above tie to the oracle."""
    renderer.set_scene(sim.scene(oracle))
    fb = lib.make_feedback(THR, LO, HI)
    start = edited(START)
    frames = []
    for with_halves in (False, True):
        with renderer.sample_map(W, H) as smap:
            set_map(torch, smap, start)
            err = torch.full((len(start), 2), -1, dtype=torch.int64, device="cuda")
            if with_halves:
                bufs, _ = queue_feedback_halves(lib, renderer, torch, oracle, smap, W, H, fb, err=err)
            else:
                bufs = sentinels(torch, W, H)
                renderer.render_sample_map_feedback(rci_of(lib, oracle, MAX, W, H), bufs[0], bufs[1], smap, fb,
                                                    sample_count=bufs[2], options=lib.make_options(rng_mode=HASH),
                                                    tile_error=err)
            torch.cuda.synchronize()
            frames.append(to_host(bufs) + (err.cpu().numpy(), smap.debug_feedback()["next"]))
    for plain, halves in zip(*frames):
        assert plain.tobytes() == halves.tobytes()
    counts = texel_counts(hs.even_table(start), W, H)
    assert_exact(frames[0][:3], counts, sim.expected_frame(oracle, counts))
    plain = ta.gpu_adaptive(lib, renderer, torch, oracle, W, H, set_scene=False)
    halves, _ = gpu_adaptive_halves(lib, renderer, torch, oracle, W, H)
    for p, h in zip(plain[:3], halves[:3]):
        assert p.tobytes() == h.tobytes()
    assert bytes(plain[3]) == bytes(halves[3])


@pytest.mark.gpu
def test_refusals_leave_the_outputs_alone(lib, renderer, torch, oracle):
    """Each refusal of rt_half_outputs through the two context-taking calls: RT_ERR_INVALID_ARGUMENT
    naming the field, nothing queued (every output keeps its sentinels), and the next frame is exact."""
    from rtvk import abi
    renderer.set_scene(sim.scene(oracle))
    c = abi.load_library()
    bufs, hb = sentinels(torch, W, H), half_sentinels(torch, W, H)
    acc, a, b, hc = bufs[0].data_ptr(), hb[0].data_ptr(), hb[1].data_ptr(), hb[2].data_ptr()
    rci = rci_of(lib, oracle, MAX, W, H)
    opt = lib.make_options(rng_mode=HASH)
    ad, info, fb = lib.make_adaptive(ta.THR, ta.MIN, ta.STEP), abi.AdaptiveInfo(), lib.make_feedback(THR, LO, HI)
    cases = [(None, "halves is NULL"), ((None, b, hc, None), "accum_a is NULL"), ((a, None, hc, None), "accum_b is NULL"),
             ((a, b, hc, 8), "reserved"), ((a, a, hc, None), "accum_a and accum_b"),
             ((acc, b, hc, None), "accum_a is accum_rgba32f"), ((a, acc, hc, None), "accum_b is accum_rgba32f")]
    with renderer.sample_map(W, H) as smap:
        set_map(torch, smap, START)
        for fields, name in cases:
            ref = None
            if fields is not None:
                s = abi.HalfOutputs()
                s.accum_a, s.accum_b, s.half_count, s.reserved = fields
                ref = ctypes.byref(s)
            for rc in (c.rt_render_adaptive_halves_device(renderer._ctx, ctypes.byref(rci), None, W, H, acc,
                                                          bufs[1].data_ptr(), bufs[2].data_ptr(), ctypes.byref(opt),
                                                          ctypes.byref(ad), ctypes.byref(info), ref, None),
                       c.rt_render_sample_map_feedback_halves_device(renderer._ctx, ctypes.byref(rci), None, W, H, acc,
                                                                     bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                                     ctypes.byref(opt), smap._map, ctypes.byref(fb), None,
                                                                     ref, None)):
                assert rc == -1 and name in c.rt_last_error().decode(), (name, rc, c.rt_last_error())
        # the plain calls' refusals come through the halves calls too
        with pytest.raises(lib.RtError, match="must be even"):
            renderer.render_sample_map_feedback(rci_of(lib, oracle, 65, W, H), bufs[0], bufs[1], smap, fb,
                                                options=opt, accum_a=hb[0], accum_b=hb[1], half_count=hb[2])
        with pytest.raises(lib.RtError, match="rng_mode"):
            renderer.render_adaptive(rci, bufs[0], bufs[1], options=lib.make_options(), adaptive=ad, accum_a=hb[0],
                                     accum_b=hb[1], half_count=hb[2])
        torch.cuda.synchronize()
        assert float((bufs[0] + 1.0).abs().sum()) == 0.0 and int((bufs[1] != 7).sum()) == 0
        assert int((bufs[2] != -1).sum()) == 0 and int((hb[2] != -1).sum()) == 0
        assert float((hb[0] + 1.0).abs().sum()) == 0.0 and float((hb[1] + 1.0).abs().sum()) == 0.0
        # and the Python layer's own
        with pytest.raises(ValueError, match="accum_a and accum_b"):
            renderer.render_adaptive(rci, bufs[0], bufs[1], options=opt, adaptive=ad, accum_a=hb[0])
        with pytest.raises(ValueError, match="half_count"):
            renderer.render_adaptive(rci, bufs[0], bufs[1], options=opt, adaptive=ad, accum_a=hb[0], accum_b=hb[1],
                                     half_count=hb[2].to(torch.float32))
    adaptive_parity(lib, renderer, torch, oracle, W, H)
