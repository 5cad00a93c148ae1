"""The block table of a one-launch sample-map frame (rt_sample_map_block_plan, csrc/rt_sample_map.cpp,
DESIGN.md §3.1.2) on the CPU, against a few lines of Python: the tiles in sample_map_plan's order
without the zero tiles, a tile of count n in k = ceil(n / U) chunks [c n // k, (c + 1) n // k); the
automatic unit; the refusals with their outputs untouched; a table of 71 levels, which the level plan
refuses and the block plan takes; the new symbols. No GPU."""
import ctypes

import numpy as np
import pytest

EXAMPLE = [0, 1, 2, 7, 8, 64, 64, 3, 0, 0, 5, 12, 12, 1, 2, 2, 9, 9, 9, 30, 0, 64, 7, 8]
MAX_COUNT = 1 << 19
LANES = 256 * 1536   # the nominal lanes of the automatic unit (rt_sample_map.h kNominalLanes)


@pytest.fixture(scope="module")
def lib(oracle):
    import rtvk
    return rtvk


def restated(lib, counts, quantum=0, unit=0):
    """(blocks as a list of (tile, s0, s1, 0), U): the definition, in Python integers."""
    q = max(1, quantum)
    n = [(int(c) + q - 1) // q * q for c in counts]
    if unit == 0:
        floor = min(128, max(32, max(n, default=0) // 32))
        unit = max(floor, -(-sum(64 * c for c in n) // (LANES * 128)))
    order = np.lexsort((np.arange(len(n)), -np.asarray(n, np.int64))).tolist() if n else []   # count descending, tile ascending
    if len(set(n) - {0}) <= 64:   # sample_map_plan's order, where the level plan takes the table
        assert lib.sample_map_plan(counts, quantum)["order"].tolist() == order
    blocks = []
    for t in order:
        if n[t] == 0:
            continue
        k = -(-n[t] // unit)
        blocks += [(t, c * n[t] // k, (c + 1) * n[t] // k, 0) for c in range(k)]
    return blocks, unit, n, order


def check_case(lib, counts, quantum=0, unit=0):
    got = lib.sample_map_block_plan(counts, quantum, unit)
    want, U, n, order = restated(lib, counts, quantum, unit)
    b = got["blocks"]
    assert b.dtype == np.uint32 and b.shape == (len(want), 4) and got["unit_samples"] == U
    assert [tuple(r) for r in b.tolist()] == want
    # the properties, from the library's table alone
    assert (b[:, 3] == 0).all()
    tiles = b[:, 0].tolist()
    live = [t for t in order if n[t] > 0]
    assert [t for i, t in enumerate(tiles) if i == 0 or tiles[i - 1] != t] == live   # the order, zero tiles absent
    assert len(b) == sum(-(-n[t] // U) for t in live)
    for t in live:
        rows = b[b[:, 0] == t]
        assert len(rows) == -(-n[t] // U)                                  # k = ceil(n / U)
        assert rows[0, 1] == 0 and rows[-1, 2] == n[t]                     # a partition of [0, n) ...
        assert (rows[1:, 1] == rows[:-1, 2]).all()                         # ... in order
        size = rows[:, 2].astype(np.int64) - rows[:, 1]
        assert size.min() >= 1 and size.max() <= U
    return got


@pytest.mark.parametrize("unit", [1, 3, 5, 64, 1 << 19, 0])
def test_worked_example(lib, unit):
    got = check_case(lib, EXAMPLE, unit=unit)
    if unit == 0:
        assert got["unit_samples"] == 32   # the floor: clamp(64 / 32, 32, 128)
    if unit >= 64:
        assert len(got["blocks"]) == 20    # one block per non-zero tile


def test_worked_example_quantum_16(lib):
    for unit in (0, 5, 16):
        check_case(lib, EXAMPLE, quantum=16, unit=unit)


def test_spot_value(lib):
    """n = 7 at U = 3: three chunks [0, 2), [2, 4), [4, 7)."""
    b = lib.sample_map_block_plan(EXAMPLE, 0, 3)["blocks"]
    assert b[b[:, 0] == 3].tolist() == [[3, 0, 2, 0], [3, 2, 4, 0], [3, 4, 7, 0]]
    assert lib.sample_map_block_plan([7], 0, 3)["blocks"].tolist() == [[0, 0, 2, 0], [0, 2, 4, 0], [0, 4, 7, 0]]


def test_random_tables(lib):
    rng = np.random.default_rng(20241019)
    for n_tiles, hi in ((1, 9), (24, 64), (1000, 300)):
        for unit in (0, 1, 7, 40):
            check_case(lib, rng.integers(0, hi + 1, n_tiles), unit=unit)
    check_case(lib, rng.integers(0, 10001, 1000), quantum=512)
    check_case(lib, [0] * 24)
    check_case(lib, [])
    assert lib.sample_map_block_plan([0] * 24)["blocks"].shape == (0, 4)


def test_automatic_unit_follows_the_total(lib):
    """32 400 tiles (1080p) of 10 000 samples: ceil(64 * 3.24e8 / (393 216 * 128)) = 412 > the floor 128."""
    got = lib.sample_map_block_plan([10000] * 32400)
    assert got["unit_samples"] == 412 and got["blocks"].shape == (32400 * 25, 4)   # k = ceil(10 000 / 412) = 25
    b = got["blocks"].reshape(32400, 25, 4)
    assert (b[:, :, 0] == np.arange(32400)[:, None]).all()
    assert (b[:, :, 1] == np.arange(25) * 10000 // 25).all() and (b[:, :, 2] == np.arange(1, 26) * 10000 // 25).all()
    assert check_case(lib, [4096] * 24)["unit_samples"] == 128   # the floor 4096 / 32
    assert check_case(lib, [2048] * 24)["unit_samples"] == 64


def test_71_levels(lib):
    from rtvk import RtError
    table = [1 + (29 * t) % 71 for t in range(72)]
    assert len(set(table)) == 71
    with pytest.raises(RtError) as e:
        lib.sample_map_plan(table)
    assert e.value.code == -1 and "71 levels" in str(e.value)
    for unit in (0, 1, 5):
        check_case(lib, table, unit=unit)


def raw_call(lib, counts, quantum, unit, capacity=8):
    """The C call with sentinel outputs: (rc, blocks, n_blocks, unit_used, message)."""
    c = np.ascontiguousarray(counts, np.uint32)
    blocks = np.full((capacity, 4), 0xdead, np.uint32)
    nb, used = ctypes.c_uint64(0xdead), ctypes.c_uint32(0xdead)
    L = lib.load_library()
    rc = L.rt_sample_map_block_plan(c.ctypes.data, len(c), quantum, unit, blocks.ctypes.data, capacity, ctypes.byref(nb),
                                    ctypes.byref(used))
    return rc, blocks, nb.value, used.value, L.rt_last_error().decode()


def assert_refused(res, needle):
    rc, blocks, nb, used, msg = res
    assert rc == -1 and needle in msg, msg
    assert (blocks == 0xdead).all() and nb == 0xdead and used == 0xdead   # nothing written


def test_refusals_leave_outputs_untouched(lib):
    assert_refused(raw_call(lib, [3, 7, MAX_COUNT + 1, 0xffffffff], 0, 0), "tile_counts[2]")
    assert_refused(raw_call(lib, [5, MAX_COUNT - 1], 3, 0), "tile_counts[1]")
    assert_refused(raw_call(lib, [5, 6], 0, MAX_COUNT + 1), "unit_samples")
    # 64 tiles of 2^19 samples at U = 1: 2^25 blocks, one too many for unit ids of 32 bits; U = 2 fits
    res = raw_call(lib, [MAX_COUNT] * 64, 0, 1)
    assert_refused(res, "unit_samples that fits is 2")
    assert "33554432 blocks" in res[4]
    assert_refused(raw_call(lib, [5, 6], 0, 1, capacity=10), "capacity")      # 11 blocks
    rc, blocks, nb, used, _ = raw_call(lib, [5, 6], 0, 1, capacity=11)
    assert rc == 0 and nb == 11 and used == 1 and (blocks[:, 3] == 0).all()
    L = lib.load_library()
    assert L.rt_sample_map_block_plan(None, 3, 0, 0, None, 0, None, None) == -1   # NULL table
    assert L.rt_sample_map_block_plan(None, 0, 0, 0, None, 0, None, None) == 0    # every output NULL


def test_the_2_to_25_block_case_fits_at_the_automatic_unit_and_at_2(lib):
    """The automatic unit is doubled until the table fits: at this table it starts at 128 and already
    fits (2^18 blocks); U = 2, the unit the refusal names, gives 2^24."""
    L = lib.load_library()
    c = np.full(64, MAX_COUNT, np.uint32)
    nb, used = ctypes.c_uint64(0), ctypes.c_uint32(0)
    assert L.rt_sample_map_block_plan(c.ctypes.data, 64, 0, 0, None, 0, ctypes.byref(nb), ctypes.byref(used)) == 0
    assert (used.value, nb.value) == (128, 64 * 4096) and 64 * nb.value < 1 << 31
    assert L.rt_sample_map_block_plan(c.ctypes.data, 64, 0, 2, None, 0, ctypes.byref(nb), ctypes.byref(used)) == 0
    assert (used.value, nb.value) == (2, 1 << 24)


def test_symbols_and_abi(lib):
    from rtvk import abi
    L = lib.load_library()
    for name in ("rt_sample_map_set_schedule", "rt_sample_map_get_schedule", "rt_sample_map_block_plan",
                 "rt_debug_sample_map_blocks"):
        assert name in abi.EXPORTS and getattr(L, name) is not None
    assert L.rt_abi_version() == 2
    assert (abi.SAMPLE_MAP_LEVELS, abi.SAMPLE_MAP_ONE_LAUNCH) == (0, 1)
    for method in ("schedule", "schedule_info", "debug_blocks"):
        assert callable(getattr(lib.SampleMap, method))
