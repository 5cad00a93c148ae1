"""Adaptive frames across devices (rt_multi_render_adaptive): the tile-row
partition and the frame plan on the CPU, and on the GPU the N-device adaptive frame, executed over
logical devices on GPU 0, against the pass loop simulated on the unchanged oracle (adaptive_sim.py),
against the one-device adaptive frame and against plain multi-device frames.

The standard of proof is test_adaptive.py's: sample s of a pixel is a pure function of
(pixel_seed, s) and sums are integers, so the N-device frame must equal the one-device frame bit for
bit, and a tile that stopped at n samples holds oracle.render(spp=n) on every texel.
"""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402

HASH = 2
MIN, STEP, MAX, THR = 8, 8, 64, 0.2     # tests/test_adaptive.py's constants
INVALID_ARGUMENT, NO_SCENE = -1, -4
GOLDEN = Path(__file__).resolve().parent / "golden" / "multi_plan_v1.json"
PLAN_SHAPES = [(1, 44, 27), (2, 44, 27), (3, 64, 40), (8, 44, 27)]


@pytest.fixture(scope="module")
def rtvk():
    import rtvk as m
    m.load_library()
    return m


# ---- CPU: the partition ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 13])
def test_partition_tile_rows(rtvk, n):
    for H in (1, 7, 8, 9, 27, 40, 1080, 2160):
        parts = rtvk.partition_tile_rows(n, H)
        T = (H + 7) // 8
        assert len(parts) == n
        allrows = np.concatenate(parts)
        assert sorted(allrows.tolist()) == list(range(H)), (n, H)           # every row exactly once
        for d, rows in enumerate(parts):
            rows = rows.astype(np.int64)
            if d >= T:
                assert len(rows) == 0, (n, H, d)                             # no tile row: nothing
                continue
            assert (np.diff(rows) > 0).all(), (n, H, d)                      # ascending
            # whole aligned 8-row groups, in order: band tile row j is global tile row d + j n
            ks = list(range(d, T, n))
            want = np.concatenate([np.arange(8 * k, min(8 * k + 8, H)) for k in ks])
            assert np.array_equal(rows, want), (n, H, d)
            assert ((rows // 8) % n == d).all()                              # tile row k on device k % n
            groups = [rows[8 * j:8 * j + 8] for j in range(len(ks))]
            for j, g in enumerate(groups):
                assert g[0] % 8 == 0
                assert len(g) == 8 or (ks[j] == T - 1 and j == len(groups) - 1), (n, H, d)   # ragged: last only


def test_partition_tile_rows_refusals(rtvk):
    lib = rtvk.load_library()
    rows = (ctypes.c_uint32 * 64)()
    counts = (ctypes.c_uint32 * 4)()
    for args in ((0, 27, rows, counts), (2, 27, None, counts), (2, 27, rows, None)):
        assert lib.rt_partition_tile_rows(*args) == INVALID_ARGUMENT
        assert lib.rt_last_error()
    assert lib.rt_partition_tile_rows(2, 0, rows, counts) == 0 and list(counts[:2]) == [0, 0]   # as the strips


# ---- CPU: the plan ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,W,H", PLAN_SHAPES)
def test_adaptive_plan(rtvk, n, W, H):
    plan = rtvk.multi_plan_adaptive(n, W, H)
    parts, steps = plan["parts"], plan["steps"]
    want = [r for r in rtvk.partition_tile_rows(n, H) if len(r)]
    assert len(parts) == len(want) == min(n, (H + 7) // 8)                   # a device without tile rows: no part
    for d, (dev, whole, rows) in enumerate(parts):
        assert dev == d and np.array_equal(rows, want[d]) and whole == (n == 1)
    ops = [s["op"] for s in steps]
    assert "resolve" not in ops and "store_rows" not in ops and "render" not in ops and "load_rows" not in ops
    assert all(s["dev"] < len(parts) and s["peer"] < len(parts) and s["part"] < len(parts) for s in steps)
    renders = [s for s in steps if s["op"] == "render_adaptive"]
    assert [s["part"] for s in renders] == list(range(len(parts)))
    assert ops[:len(renders)] == ["render_adaptive"] * len(renders)          # every part's passes lead the plan
    if n == 1:
        assert len(steps) == 1 and renders[0]["flags"] == 1 and renders[0]["dev"] == 0   # direct, no transfers
        return
    assert all(s["flags"] == 0 and s["dev"] == parts[s["part"]][0] for s in renders)
    # one group: per remote part one accumulator pair and one count pair; device 0's part is not sent
    assert ops.count("group_start") == ops.count("group_end") == 1
    g0, g1 = ops.index("group_start"), ops.index("group_end")
    inside = steps[g0 + 1:g1]
    assert all(s["op"] in ("send", "recv", "send_counts", "recv_counts") for s in inside)
    assert not any(s["op"] in ("send", "recv", "send_counts", "recv_counts") for s in steps[:g0] + steps[g1 + 1:])
    for p, (dev, _, rows) in enumerate(parts):
        mine = [s for s in inside if s["part"] == p]
        if dev == 0:
            assert mine == []
            continue
        floats, words = len(rows) * W * 4, ((W + 7) // 8) * ((len(rows) + 7) // 8)
        assert [(s["op"], s["dev"], s["peer"], s["count"]) for s in mine] == [
            ("send", dev, 0, floats), ("recv", 0, dev, floats),
            ("send_counts", dev, 0, words), ("recv_counts", 0, dev, words)]
    stores = [s for s in steps[g1 + 1:] if s["op"] == "store_tiles"]
    assert len(stores) == len(steps) - g1 - 1
    assert [(s["part"], s["dev"], s["count"]) for s in stores] == \
        [(p, 0, len(rows) * W * 4) for p, (_, _, rows) in enumerate(parts)]     # one store per part


def test_adaptive_plan_refusals(rtvk):
    lib = rtvk.load_library()
    n = ctypes.c_uint64(0)
    for args in ((0, 44, 27), (2, 0, 27), (2, 44, 0)):
        assert lib.rt_debug_multi_plan_adaptive(*args, None, 0, ctypes.byref(n)) == INVALID_ARGUMENT
    assert lib.rt_debug_multi_plan_adaptive(2, 44, 27, None, 0, None) == INVALID_ARGUMENT
    assert lib.rt_debug_multi_plan_adaptive(2, 44, 27, None, 0, ctypes.byref(n)) == 0 and n.value > 0
    buf = (ctypes.c_uint32 * n.value)()
    assert lib.rt_debug_multi_plan_adaptive(2, 44, 27, buf, n.value - 1, ctypes.byref(n)) == INVALID_ARGUMENT


def test_existing_plans_unchanged(rtvk):
    """rt_debug_multi_plan's words for the shapes above, with and without accumulation, against the
    table recorded from the commit before the adaptive ops were added (tests/golden)."""
    lib = rtvk.load_library()
    table = json.loads(GOLDEN.read_text())["plans"]
    assert sorted({(p["n"], p["W"], p["H"]) for p in table}) == sorted(PLAN_SHAPES)
    assert len(table) == 2 * len(PLAN_SHAPES)
    for p in table:
        n = ctypes.c_uint64(0)
        args = (p["n"], p["W"], p["H"], None, 0, p["accumulate"])
        assert lib.rt_debug_multi_plan(*args, None, 0, ctypes.byref(n)) == 0
        buf = (ctypes.c_uint32 * n.value)()
        assert lib.rt_debug_multi_plan(*args, buf, n.value, ctypes.byref(n)) == 0
        assert list(buf) == p["words"], (p["n"], p["W"], p["H"], p["accumulate"])


# ---- GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(oracle, rtvk):
    return rtvk


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


_REF = {}


def reference(lib, oracle, W, H, k=11, thr=THR):
    """(Q, counts, info, (accum, rgba8)) of the one-device frame, once per shape and scene."""
    key = (W, H, k, thr)
    if key not in _REF:
        Q = sim.cube(oracle, W, H, MAX, k=k)
        counts, info = sim.simulate(Q, MIN, STEP, MAX, lib.threshold_q16(thr))
        sim.assert_not_vacuous(counts, MAX)
        ref = sim.expected_frame(oracle, counts, k=k)
        counts.setflags(write=False)
        _REF[key] = (Q, counts, info, ref)
    return _REF[key]


def rci_of(lib, oracle, W, H, spp=MAX):
    return lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, W, H).tobytes())


def sentinels(torch, W, H):
    return (torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0"),
            torch.full((H, W, 4), 7, dtype=torch.uint8, device="cuda:0"),
            torch.full((H, W), -1, dtype=torch.int32, device="cuda:0"))


def multi_adaptive(lib, m, torch, oracle, W, H, thr=THR, mx=MAX):
    acc, out, cnt = sentinels(torch, W, H)
    info = m.render_adaptive(rci_of(lib, oracle, W, H, mx), acc, out, sample_count=cnt,
                             options=lib.make_options(rng_mode=HASH), adaptive=lib.make_adaptive(thr, MIN, STEP))
    torch.cuda.synchronize()
    return acc.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), info


def multi_plain(lib, m, torch, oracle, W, H, spp):
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    m.render(rci_of(lib, oracle, W, H, spp), acc, out, options=lib.make_options(rng_mode=HASH))
    torch.cuda.synchronize()
    return acc.cpu().numpy(), out.cpu().numpy()


def info_tuple(i):
    return (i.passes, i.tiles, i.tiles_capped, i.samples, i.reserved)


def assert_parity(lib, m, got, n, W, H, Q, counts, info_sim, ref):
    """The frame against the simulation and the oracle, and each device's numbers against the
    simulation of its own rows (band tile row j of a part is one global tile row)."""
    acc, out, cnt, info = got
    np.testing.assert_array_equal(cnt, counts)
    bad = np.argwhere(acc != ref[0])
    assert bad.size == 0, f"{len(bad)} accumulator floats differ, first at {bad[:4].tolist()}"
    np.testing.assert_array_equal(out, ref[1])
    assert info_tuple(info) == (info_sim["passes"], info_sim["tiles"], info_sim["tiles_capped"], info_sim["samples"], 0)
    devs = [m.adaptive_device_info(d) for d in range(n)]
    assert max(d.passes for d in devs) == info.passes
    assert sum(d.tiles for d in devs) == info.tiles and sum(d.samples for d in devs) == info.samples
    assert sum(d.tiles_capped for d in devs) == info.tiles_capped
    for d, rows in enumerate(lib.partition_tile_rows(n, H)):
        if len(rows) == 0:
            assert info_tuple(devs[d]) == (0, 0, 0, 0, 0)                    # rendered nothing
            continue
        _, s = sim.simulate(Q[:, rows], MIN, STEP, MAX, lib.threshold_q16(THR))
        assert info_tuple(devs[d]) == (s["passes"], s["tiles"], s["tiles_capped"], s["samples"], 0), d


@pytest.mark.gpu
@pytest.mark.parametrize("logical,n,W,H", [(True, 2, 44, 27), (True, 3, 44, 27), (True, 8, 44, 27),
                                           ("rccl", 2, 64, 40)])
def test_parity_with_simulation_and_oracle(lib, torch, oracle, logical, n, W, H):
    """Ragged width, a ragged last tile row, idle devices (8 devices, 4 tile rows), and the RCCL
    transport of a one-rank communicator."""
    Q, counts, info_sim, ref = reference(lib, oracle, W, H)
    with lib.MultiRenderer(n, logical=logical) as m:
        m.set_scene(sim.scene(oracle))
        got = multi_adaptive(lib, m, torch, oracle, W, H)
        assert_parity(lib, m, got, n, W, H, Q, counts, info_sim, ref)
        assert m.info()["rccl_ranks"] == (1 if logical == "rccl" else 0)


@pytest.mark.gpu
def test_equals_one_device(lib, torch, oracle):
    W, H = 44, 27
    with lib.Renderer(0) as r:
        r.set_scene(sim.scene(oracle))
        acc, out, cnt = sentinels(torch, W, H)
        i1 = r.render_adaptive(rci_of(lib, oracle, W, H), acc, out, sample_count=cnt,
                               options=lib.make_options(rng_mode=HASH), adaptive=lib.make_adaptive(THR, MIN, STEP))
        torch.cuda.synchronize()
        one = (acc.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32))
    for n, logical in ((3, True), (1, False)):      # three logical devices; one device: the direct path
        with lib.MultiRenderer(n, logical=logical) as m:
            m.set_scene(sim.scene(oracle))
            a, o, c, i = multi_adaptive(lib, m, torch, oracle, W, H)
            assert np.array_equal(a, one[0]) and np.array_equal(o, one[1]) and np.array_equal(c, one[2]), n
            assert info_tuple(i) == info_tuple(i1), n
            if n == 1:
                assert info_tuple(m.adaptive_device_info(0)) == info_tuple(i1)


@pytest.mark.gpu
def test_anchors_without_the_oracle(lib, torch, oracle):
    """Threshold 0 is the uniform 64-spp multi-device frame, threshold 16 the 8-spp frame."""
    W, H, n = 44, 27, 3
    with lib.MultiRenderer(n, logical=True) as m:
        m.set_scene(sim.scene(oracle))
        a, o, c, i = multi_adaptive(lib, m, torch, oracle, W, H, thr=0.0)
        pa, po = multi_plain(lib, m, torch, oracle, W, H, MAX)
        assert np.array_equal(a, pa) and np.array_equal(o, po)
        assert (c == MAX).all() and i.passes == 8 and i.tiles_capped == i.tiles == 24 and i.samples == MAX * W * H
        a, o, c, i = multi_adaptive(lib, m, torch, oracle, W, H, thr=16.0)
        pa, po = multi_plain(lib, m, torch, oracle, W, H, MIN)
        assert np.array_equal(a, pa) and np.array_equal(o, po)
        assert (c == MIN).all() and i.passes == 1 and i.tiles_capped == 0 and i.samples == MIN * W * H


@pytest.mark.gpu
def test_hygiene_with_plain_frames(lib, torch, oracle):
    """An adaptive frame leaves the plain frames' partition, balancer and images alone; adaptive
    frames repeat; the image size may change between them."""
    W, H, n = 44, 27, 3
    Q, counts, info_sim, ref = reference(lib, oracle, W, H)
    with lib.MultiRenderer(n, logical=True) as m:
        m.set_scene(sim.scene(oracle))
        p1 = multi_plain(lib, m, torch, oracle, W, H, 6)
        part = [r.tolist() for r in m.partition(H)]
        bal = m.balance_info()
        a1 = multi_adaptive(lib, m, torch, oracle, W, H)
        assert [r.tolist() for r in m.partition(H)] == part
        assert m.balance_info() == bal
        assert_parity(lib, m, a1, n, W, H, Q, counts, info_sim, ref)
        p3 = multi_plain(lib, m, torch, oracle, W, H, 6)
        assert np.array_equal(p3[0], p1[0]) and np.array_equal(p3[1], p1[1])
        a2 = multi_adaptive(lib, m, torch, oracle, W, H)
        for x, y in zip(a1[:3], a2[:3]):
            assert np.array_equal(x, y)
        assert info_tuple(a1[3]) == info_tuple(a2[3])
        big = multi_adaptive(lib, m, torch, oracle, 64, 40)                  # another size, and back
        assert_parity(lib, m, big, n, 64, 40, *reference(lib, oracle, 64, 40))
        a3 = multi_adaptive(lib, m, torch, oracle, W, H)
        assert_parity(lib, m, a3, n, W, H, Q, counts, info_sim, ref)


@pytest.mark.gpu
def test_device_built_scene(lib, torch, oracle):
    """1 160 spheres (k = 17): each logical device's own device build, its L2 grid / treelet walks."""
    W, H, n = 44, 27, 2
    Q, counts, info_sim, ref = reference(lib, oracle, W, H, k=17)
    with lib.MultiRenderer(n, logical=True) as m:
        m.set_scene(sim.scene(oracle, 17))
        got = multi_adaptive(lib, m, torch, oracle, W, H)
        assert_parity(lib, m, got, n, W, H, Q, counts, info_sim, ref)


@pytest.mark.gpu
def test_refusals(lib, torch, oracle):
    from rtvk import RtError, abi
    W, H, n = 44, 27, 2
    acc, out, cnt = sentinels(torch, W, H)
    raw = lib.load_library()

    def untouched():
        torch.cuda.synchronize()
        assert bool((acc == -1.0).all()) and bool((out == 7).all()) and bool((cnt == -1).all())

    def refused(m, field, code=INVALID_ARGUMENT, spp=MAX, ad=None, **opt):
        o = dict(rng_mode=HASH)
        o.update(opt)
        with pytest.raises(RtError) as e:
            m.render_adaptive(rci_of(lib, oracle, W, H, spp), acc, out, sample_count=cnt,
                              options=lib.make_options(**o), adaptive=ad or lib.make_adaptive(THR, MIN, STEP))
        assert e.value.code == code and field in str(e.value), str(e.value)

    with lib.MultiRenderer(n, logical=True) as m:
        refused(m, "rt_multi_set_scene", code=NO_SCENE)                      # before set_scene
        m.set_scene(sim.scene(oracle))
        refused(m, "rng_mode", rng_mode=abi.RT_RNG_PIXEL_STREAM)
        refused(m, "rng_mode", rng_mode=abi.RT_RNG_SAMPLE_COUNTER)
        refused(m, "accumulate", accumulate=True)
        refused(m, "min_spp", ad=lib.make_adaptive(THR, 7, 8))
        refused(m, "step_spp", ad=lib.make_adaptive(THR, 8, 3))
        refused(m, "max_spp", spp=63)
        refused(m, "min_spp", spp=4)                                         # min > max
        refused(m, "threshold", ad=lib.make_adaptive(17.0, 8, 8))
        refused(m, "threshold", ad=lib.make_adaptive(float("nan"), 8, 8))
        # NULL adaptive and NULL buffers: past the Python wrapper's own checks
        rci, opt, ad = rci_of(lib, oracle, W, H), lib.make_options(rng_mode=HASH), lib.make_adaptive(THR, MIN, STEP)
        st = torch.cuda.current_stream(0).cuda_stream
        for a_ptr, o_ptr, ad_ref in ((acc.data_ptr(), out.data_ptr(), None), (None, out.data_ptr(), ctypes.byref(ad)),
                                     (acc.data_ptr(), None, ctypes.byref(ad))):
            rc = raw.rt_multi_render_adaptive(m._m, ctypes.byref(rci), ctypes.byref(opt), ad_ref, a_ptr, o_ptr,
                                              cnt.data_ptr(), None, st)
            assert rc == INVALID_ARGUMENT and raw.rt_last_error()
        untouched()
        # and nothing left behind
        assert_parity(lib, m, multi_adaptive(lib, m, torch, oracle, W, H), n, W, H, *reference(lib, oracle, W, H))
