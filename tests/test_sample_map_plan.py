"""The plan of a sample-map frame (rt_sample_map_plan, csrc/rt_sample_map.cpp) on
the CPU: the quantised table, the tile order (count descending, tile index ascending), the levels
L_j and the prefix lengths c_j = #{t : n[t] >= L_j}, against numpy; the refusals; the totals of a
ragged band; the binding's layout. No GPU."""
import ctypes

import numpy as np
import pytest

# DESIGN.md §3.1.2's worked example: the 44x27 band, 6 x 4 tiles, row-major
EXAMPLE = [0, 1, 2, 7, 8, 64, 64, 3, 0, 0, 5, 12, 12, 1, 2, 2, 9, 9, 9, 30, 0, 64, 7, 8]
MAX_COUNT = 1 << 19


@pytest.fixture(scope="module")
def lib(oracle):
    import rtvk
    return rtvk


def reference_plan(counts, quantum=0):
    """The plan in numpy: np.lexsort's last key is the primary one."""
    n = np.asarray(counts, np.int64)
    q = max(1, quantum)
    n = (n + q - 1) // q * q
    order = np.lexsort((np.arange(len(n)), -n))
    levels = np.unique(n[n > 0])
    level_tiles = np.array([(n >= L).sum() for L in levels], np.int64)
    return {"order": order, "levels": levels, "level_tiles": level_tiles, "quantised": n}


def assert_plan(got, ref):
    for k in ("order", "levels", "level_tiles", "quantised"):
        assert got[k].dtype == np.uint32
        np.testing.assert_array_equal(got[k].astype(np.int64), ref[k], err_msg=k)


def test_worked_example(lib):
    p = lib.sample_map_plan(EXAMPLE)
    assert p["levels"].tolist() == [1, 2, 3, 5, 7, 8, 9, 12, 30, 64]
    assert p["level_tiles"].tolist() == [20, 18, 15, 14, 13, 11, 9, 6, 4, 3]
    assert p["order"].tolist() == [5, 6, 21, 19, 11, 12, 16, 17, 18, 4, 23, 3, 22, 10, 7, 2, 14, 15, 1, 13, 0, 8, 9, 20]
    assert p["quantised"].tolist() == EXAMPLE
    assert_plan(p, reference_plan(EXAMPLE))


def test_worked_example_quantum_16(lib):
    p = lib.sample_map_plan(EXAMPLE, quantum=16)
    assert p["levels"].tolist() == [16, 32, 64]
    assert p["level_tiles"].tolist() == [20, 4, 3]
    assert p["quantised"].tolist() == [0 if n == 0 else -(-n // 16) * 16 for n in EXAMPLE]
    assert_plan(p, reference_plan(EXAMPLE, 16))


def test_random_tables_against_lexsort(lib):
    rng = np.random.default_rng(20240907)
    for n_tiles, hi, quantum in ((1, 4, 0), (2, 3, 0), (7, 5, 2), (24, 64, 0), (375, 7, 0), (375, 40, 3), (4096, 60, 0),
                                 (32400, 10000, 512), (32400, 64, 1)):
        for _ in range(3):
            counts = rng.integers(0, hi + 1, n_tiles)
            counts[rng.random(n_tiles) < 0.2] = 0
            assert_plan(lib.sample_map_plan(counts, quantum), reference_plan(counts, quantum))


def test_one_tile_zero_table_and_equal_counts(lib):
    p = lib.sample_map_plan([5])
    assert (p["order"].tolist(), p["levels"].tolist(), p["level_tiles"].tolist()) == ([0], [5], [1])
    p = lib.sample_map_plan([0])
    assert (p["order"].tolist(), p["levels"].tolist(), p["level_tiles"].tolist()) == ([0], [], [])
    p = lib.sample_map_plan(np.zeros(24, np.uint32))
    assert len(p["levels"]) == 0 and len(p["level_tiles"]) == 0 and p["order"].tolist() == list(range(24))
    p = lib.sample_map_plan(np.full(24, 6, np.uint32))
    assert p["levels"].tolist() == [6] and p["level_tiles"].tolist() == [24] and p["order"].tolist() == list(range(24))
    p = lib.sample_map_plan([])   # no tile: an empty plan
    assert len(p["order"]) == 0 and len(p["levels"]) == 0


def test_level_limit(lib):
    from rtvk import RtError
    counts = np.arange(0, 65)   # 0 and 1 .. 64: exactly 64 levels
    p = lib.sample_map_plan(counts)
    assert p["levels"].tolist() == list(range(1, 65)) and p["level_tiles"].tolist() == list(range(64, 0, -1))
    assert_plan(p, reference_plan(counts))
    with pytest.raises(RtError) as e:
        lib.sample_map_plan(np.arange(0, 66))
    assert e.value.code == -1 and "65 levels" in str(e.value) and "quantum" in str(e.value)
    assert len(lib.sample_map_plan(np.arange(0, 66), quantum=2)["levels"]) == 33   # the quantum it suggests


def test_count_limit(lib):
    from rtvk import RtError
    p = lib.sample_map_plan([3, MAX_COUNT, 0])
    assert p["levels"].tolist() == [3, MAX_COUNT] and p["order"].tolist() == [1, 0, 2]
    with pytest.raises(RtError) as e:
        lib.sample_map_plan([3, 7, MAX_COUNT + 1, 0xffffffff])
    assert e.value.code == -1 and "tile_counts[2]" in str(e.value) and "2^19" in str(e.value)
    # a quantum that pushes a count past 2^19: 2^19 - 1 rounds up to 3 * 174763 = 2^19 + 1
    assert len(lib.sample_map_plan([5, MAX_COUNT - 1])["levels"]) == 2
    with pytest.raises(RtError) as e:
        lib.sample_map_plan([5, MAX_COUNT - 1], quantum=3)
    assert e.value.code == -1 and "tile_counts[1]" in str(e.value) and "quantum" in str(e.value)
    assert lib.sample_map_plan([5, MAX_COUNT - 1], quantum=2)["quantised"].tolist() == [6, MAX_COUNT]
    # a huge quantum does not wrap
    with pytest.raises(RtError):
        lib.sample_map_plan([1], quantum=0xffffffff)


def test_quantum_zero_is_quantum_one(lib):
    a, b = lib.sample_map_plan(EXAMPLE, 0), lib.sample_map_plan(EXAMPLE, 1)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_totals_of_a_ragged_band(lib):
    """44x27: tile columns 0-4 are 8 wide and column 5 is 4; tile rows 0-2 are 8 high and row 3 is 3:
    edge tiles have 32, 24 or 12 in-band pixels."""
    W, H = 44, 27
    n = np.array(EXAMPLE, np.int64).reshape(4, 6)
    pix = np.outer([8, 8, 8, 3], [8, 8, 8, 8, 8, 4])
    assert sorted(set(pix.ravel().tolist())) == [12, 24, 32, 64]
    info = lib.sample_map_info(EXAMPLE, W, H)
    assert (info.tiles, info.levels, info.min_count, info.max_count) == (24, 10, 1, 64)
    assert info.samples == int((n * pix).sum())
    assert info.tile_launches == sum([20, 18, 15, 14, 13, 11, 9, 6, 4, 3])
    info = lib.sample_map_info(EXAMPLE, W, H, quantum=16)
    q = (n + 15) // 16 * 16
    assert (info.levels, info.min_count, info.max_count) == (3, 16, 64)
    assert info.samples == int((q * pix).sum()) and info.tile_launches == 27
    info = lib.sample_map_info(np.zeros(24, np.uint32), W, H)
    assert (info.tiles, info.levels, info.min_count, info.max_count, info.samples, info.tile_launches) == (24, 0, 0, 0, 0, 0)


def test_binding_layout(lib):
    from rtvk import abi
    assert ctypes.sizeof(abi.SampleMapInfo) == 32
    assert [getattr(abi.SampleMapInfo, f).offset for f in ("tiles", "levels", "min_count", "max_count", "samples",
                                                           "tile_launches")] == [0, 4, 8, 12, 16, 24]
    assert abi.SAMPLE_MAP_MAX_LEVELS == 64 and abi.SAMPLE_MAP_MAX_COUNT == MAX_COUNT
    for name in ("rt_sample_map_create", "rt_sample_map_destroy", "rt_sample_map_set_device",
                 "rt_sample_map_set_from_adaptive", "rt_sample_map_get_info", "rt_render_sample_map_device",
                 "rt_sample_map_plan", "rt_debug_sample_map"):
        assert name in abi.EXPORTS and hasattr(lib.load_library(), name)
    assert lib.load_library().rt_abi_version() == 2
