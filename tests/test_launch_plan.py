"""The single-device launch plan (csrc/rt_launch.{h,cpp}) on the CPU: every host decision that
shapes a trace launch — kernel form and LDS bytes, cull slack, sample chunks, the head / tail split
of the LPT order, the block hand-out — computed through rt_debug_launch_plan without a context, and
the per-row weights of rt_launch_row_weights through rt_debug_row_weights.

tests/golden/launch_plan_v1.json holds the plans the code produced when it was moved out of
rt_api.cpp unchanged (the commit is recorded in the file), over the matrix `cases()` builds; the
test recomputes every plan and compares every field exactly, checks the plan's invariants, and
checks three anchors that come from DESIGN.md §3.1 / §5 and BENCH_r06.json, not from the code.
`python tests/test_launch_plan.py --write COMMIT` regenerates the file.

What only the kernels' translation unit knows reaches the host-only call as tables in the inputs.
The matrix fills them with one model: 256-thread brute-force blocks, 6 per CU
(__launch_bounds__(256, 6)); 768-thread walk blocks, two per CU up to 64 KiB of dynamic LDS and one
above; and the one-layer grid form by flat_grid_form's predicate (`flat_form` below)."""
import hashlib
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "launch_plan_v1.json"

BRUTE, GRID, GRID_GLOBAL, GRID_REC = 1, 6, 7, 10   # rt_internal.h ACCEL_*
STREAM, HASH = 0, 2
ANY = 0xffffffff
OCC_MODEL = [(BRUTE, ANY, 0, ANY, 6), (0, ANY, 0, 65536, 2), (0, ANY, 65537, ANY, 1)]
CAM_R = float(np.sqrt(np.float32(13.0 * 13.0 + 11.0 * 11.0 + 3.0 * 3.0)))   # the canonical camera
F02 = float(np.float32(0.2))
PAD = float(np.float32(2120.00049))

# Scene summaries: the 488-sphere scene of configs 2 and 3 as the host SAH builder and the host grid
# lay it out, config 5's 99 860 spheres and a 1 028-sphere scene as a device build lays them out
# (Morton tree, grid walked from L2: no reference count on the host), and the edge scenes.
CANON = dict(n_spheres=488, n_big=4, n_nodes=243, n_leaf=488, has_grid=1, grid_n=(19, 1, 19), grid_n_cells=361,
             grid_n_refs=836, grid_cs=(float(np.float32(1.17204976)), float(np.float32(0.4)), float(np.float32(1.17292404))),
             small_rmin=F02, small_rmax=F02, grid_pad_radius=PAD)
SCENES = {
    "canon": CANON,
    "c5": dict(n_spheres=99860, n_big=4, n_nodes=67955, n_leaf=135912, has_grid=1, gpu_tree=1, has_treelet=1,
               grid_n=(253, 1, 253), grid_n_cells=64009, grid_n_refs=0,
               grid_cs=(float(np.float32(1.25018585)), float(np.float32(0.4)), float(np.float32(1.25017834))),
               small_rmin=F02, small_rmax=F02, grid_pad_radius=PAD),
    "dev1028": dict(n_spheres=1028, n_big=4, n_nodes=529, n_leaf=1060, has_grid=1, gpu_tree=1, has_treelet=1,
                    grid_n=(26, 1, 26), grid_n_cells=676, grid_n_refs=0,
                    grid_cs=(float(np.float32(1.24084449)), float(np.float32(0.4)), float(np.float32(1.23880279))),
                    small_rmin=F02, small_rmax=F02, grid_pad_radius=PAD),
    "empty": dict(),
    "one": dict(n_spheres=1, n_nodes=1, n_leaf=4, small_rmin=1000.0, small_rmax=1000.0),
    "nogrid": dict(CANON, has_grid=0, grid_n=(0, 0, 0), grid_n_cells=0, grid_n_refs=0, grid_cs=(0.0, 0.0, 0.0)),
    "rmin0": dict(CANON, small_rmin=0.0),
    "rminnan": dict(CANON, small_rmin=math.nan),
}
BANDS = [(8, 8, 0), (64, 36, 0), (1920, 135, 1), (1920, 1080, 0), (3840, 2160, 0), (65535, 1, 0)]   # w, h, rows map
SPPS = [1, 2, 7, 100, 1000, 10000, 1 << 19]
FORMS = [0, 6, 8, 10, 12, 14, 16, "brute"]
TUNE_OTHER = dict(grid=1, grid_scale=2, grid_coop=1, grid_cq=1, grid_rec=1, grid_full_slack=1, units_per_lane=64,
                  unit_min_samples=16, sample_chunks=7, head_chunks=2, tail_tiles_pm=500, schedule=1,
                  refill_reserve=32768, isolate_tiles=4, sah_knobs=1)


def flat_form(v, accel):
    """rt_kernels.hip flat_grid_form: the one-layer grid walk, for a launch that is not instrumented,
    of the forms that have it, over a grid one cell thick in y."""
    if accel == GRID_GLOBAL and not (v.n_big <= 4 and v.pinhole_lf):
        return 0
    return int(not (v.reserved0 & 1) and accel in (GRID, GRID_REC, GRID_GLOBAL) and v.grid_n[1] == 1)


def make_inputs(rtvk, scene, band, spp, stream, form, tune=None, lpt=1, cus=256, occ=OCC_MODEL, **more):
    w, h, rows = band
    kv = dict(SCENES[scene], cu_count=cus, band_w=w, band_h=h, has_rows=rows, spp=spp, rng_mode=stream,
              accel=1 if form == "brute" else 0, reserved1=0 if form == "brute" else form, lpt_valid=lpt,
              pinhole_lf=1, cam_r=CAM_R, block_brute=256, block_walk=768, occ=occ, **more)
    v = rtvk.launch_inputs(**kv)
    for k, x in (tune or {}).items():
        setattr(v, "tune_" + k, float(x))
    return v


def compute(rtvk, v):
    """The plan of `v` as a dict, or the library's refusal as a string. The kernel form does not
    depend on the one-layer answer, so a first plan tells which form that answer is for."""
    try:
        v.flat_grid = 0
        v.flat_grid = flat_form(v, rtvk.launch_plan(v).accel)
        return rtvk.struct_dict(rtvk.launch_plan(v))
    except rtvk.RtError as e:
        return str(e).split(": ", 1)[1]


def cases():
    """key -> keyword arguments of make_inputs."""
    out = {}

    def add(scene, band, spp, stream, form, tune, lpt):
        if stream == HASH and spp > 1 << 19:
            return
        t = "-" if not tune else ",".join(f"{k}={v}" for k, v in tune.items())
        key = f"{scene}|{band[0]}x{band[1]}{'r' if band[2] else ''}|{spp}|{'hash' if stream == HASH else 'stream'}|{form}|{t}|lpt{lpt}"
        out[key] = dict(scene=scene, band=band, spp=spp, stream=stream, form=form, tune=tune, lpt=lpt)

    full, rows = BANDS[3], BANDS[2]
    for scene in SCENES:   # every scene on every band, both streams
        for band in BANDS:
            for stream in (STREAM, HASH) if scene == "canon" else (HASH,):
                add(scene, band, 1000, stream, 0, None, 1)
    for scene, band in (("canon", full), ("c5", rows)):   # every spp, with and without an LPT order
        for spp in SPPS:
            for stream in (STREAM, HASH):
                for lpt in (0, 1):
                    add(scene, band, spp, stream, 0, None, lpt)
    for scene in ("canon", "c5", "dev1028", "nogrid"):   # every form
        for form in FORMS:
            add(scene, full, 1000, HASH, form, None, 1)
            if scene != "nogrid":
                add(scene, rows, 7, STREAM, form, None, 1)
    for key, other in TUNE_OTHER.items():   # every tuning key at 0 and at one other value
        for value in (0, other):
            add("canon", full, 10000, HASH, 0, {key: value}, 1)
            add("canon", full, 100, STREAM, 0, {key: value}, 1)
    for lpt in (0, 1):   # the frames of the anchors below (configs 2, 3 and 5)
        add("canon", full, 100, HASH, "brute", None, lpt)
        add("canon", full, 10000, HASH, 0, None, lpt)
        add("c5", BANDS[4], 1000, HASH, 0, None, lpt)
    return out


@pytest.fixture(scope="module")
def rtvk():
    import rtvk as m
    m.load_library()
    return m


def check_invariants(v, p):
    n_tiles = ((v.band_w + 7) // 8) * ((v.band_h + 7) // 8)
    assert 1 <= p["chunks"] <= max(1, min(v.spp, 4096))
    assert p["head_tiles"] <= n_tiles
    units = 64 * (p["head_tiles"] * p["head_chunks"] + (n_tiles - p["head_tiles"]) * p["chunks"])
    assert p["n_units"] == units and units < 1 << 32
    assert p["n_block_units"] % 64 == 0 and p["n_block_units"] <= p["n_units"]
    assert p["first_blocks"] <= p["n_block_units"] // 64
    assert p["isolate_blocks"] <= p["first_blocks"]
    if p["head_tiles"]:
        assert p["head_chunks"] <= p["chunks"]
    assert p["grid"] >= 1
    assert p["block"] == (256 if p["accel"] == BRUTE else 768)


def test_plans_match_the_golden_table(rtvk):
    """Every plan of the matrix, field by field, against the table recorded when the code moved."""
    gold = json.loads(GOLDEN.read_text())
    cs = cases()
    assert set(gold["cases"]) == set(cs)
    fields = gold["fields"]
    assert fields == [n for n, _ in rtvk.abi.LaunchPlan._fields_]
    bad = []
    for key, kw in cs.items():
        v = make_inputs(rtvk, **kw)
        p = compute(rtvk, v)
        want_sha, want = gold["cases"][key]
        assert hashlib.sha256(bytes(v)).hexdigest()[:8] == want_sha, f"{key}: the test's inputs changed"
        got = p if isinstance(p, str) else [p[f] for f in fields]
        if got != want:
            bad.append((key, got, want))
    assert not bad, f"{len(bad)} plans differ, first: {bad[0]}"


def test_plan_invariants(rtvk):
    """Every plan of the matrix keeps the invariants the kernels rely on; a band the plan cannot
    number in 32 bits is refused with "band too large", never planned."""
    refused = 0
    for key, kw in cases().items():
        v = make_inputs(rtvk, **kw)
        p = compute(rtvk, v)
        if isinstance(p, str):
            assert p == "band too large", (key, p)
            refused += 1
            continue
        check_invariants(v, p)
    assert refused == 0   # no band of the matrix has 2^26 tiles
    v = make_inputs(rtvk, "canon", (65535, 65535, 0), 7, HASH, 0)
    assert compute(rtvk, v) == "band too large"


def test_anchor_config3(rtvk):
    """DESIGN.md §3.1 / §5, BENCH_r06.json sample_chunks 10: config 3 (1920x1080, 10 000 spp, hash,
    grid-lds-rec) on 256 CUs with two 768-thread blocks each (393 216 lanes): 128 units per lane over
    2 073 600 pixels is 25 chunks uniform; with the LPT order, 3 head and 10 tail chunks."""
    uni = compute(rtvk, make_inputs(rtvk, "canon", (1920, 1080, 0), 10000, HASH, 0, lpt=0))
    assert (uni["accel"], uni["blocks_per_cu"], uni["block"]) == (GRID_REC, 2, 768)
    assert (uni["chunks"], uni["head_tiles"]) == (25, 0)
    lpt = compute(rtvk, make_inputs(rtvk, "canon", (1920, 1080, 0), 10000, HASH, 0, lpt=1))
    assert lpt["head_tiles"] > 0 and (lpt["head_chunks"], lpt["chunks"]) == (3, 10)


def test_anchor_config5(rtvk):
    """config 5 (3840x2160, 1 000 spp, hash) on 393 216 lanes: 7 chunks uniform; with the
    LPT order, 1 head and 3 tail chunks."""
    uni = compute(rtvk, make_inputs(rtvk, "c5", (3840, 2160, 0), 1000, HASH, 0, lpt=0))
    assert uni["blocks_per_cu"] * uni["block"] == 2 * 768
    assert (uni["chunks"], uni["head_tiles"]) == (7, 0)
    lpt = compute(rtvk, make_inputs(rtvk, "c5", (3840, 2160, 0), 1000, HASH, 0, lpt=1))
    assert lpt["head_tiles"] > 0 and (lpt["head_chunks"], lpt["chunks"]) == (1, 3)


@pytest.mark.parametrize("blocks", [5, 6, 8])
def test_anchor_config2(rtvk, blocks):
    """config 2 (brute force, 488 spheres, 1920x1080, 100 spp, hash): 20 chunks, bounded
    by spp / min_samples (units of 2560 / 488 = 5 samples), for any occupancy of at least 5 blocks
    per CU (6 by __launch_bounds__(256, 6))."""
    occ = [(BRUTE, ANY, 0, ANY, blocks)]
    for lpt in (0, 1):   # the brute-force walk records no tile costs: no order, no head
        p = compute(rtvk, make_inputs(rtvk, "canon", (1920, 1080, 0), 100, HASH, "brute", lpt=lpt, occ=occ))
        assert (p["accel"], p["block"], p["chunks"], p["head_tiles"], p["lpt"]) == (BRUTE, 256, 20, 0, 0)


def test_missing_occupancy_is_an_error(rtvk):
    """An occupancy the table does not answer fails the call: no default stands in for the kernels."""
    v = make_inputs(rtvk, "canon", (64, 36, 0), 7, HASH, 0, occ=[(BRUTE, ANY, 0, ANY, 6)])
    with pytest.raises(rtvk.RtError, match="occupancy"):
        rtvk.launch_plan(v)


@pytest.mark.parametrize("field,value", [("band_w", 0), ("band_h", 65536), ("accel", 3), ("rng_mode", 3),
                                         ("tune_sample_chunks", 1e30), ("tune_head_chunks", math.inf),
                                         ("tune_refill_reserve", math.nan), ("tune_isolate_tiles", -2.0),
                                         ("tune_units_per_lane", 2.0 ** 32 + 1024), ("version", 2), ("n_occ", 9)])
def test_inputs_outside_the_domain_are_refused(rtvk, field, value):
    v = make_inputs(rtvk, "canon", (64, 36, 0), 7, HASH, 0)
    setattr(v, field, value)
    with pytest.raises(rtvk.RtError):
        rtvk.launch_plan(v)


def test_tuning_values_up_to_2_pow_32_are_planned(rtvk):
    for key in rtvk.abi.TUNING_KEYS:
        v = make_inputs(rtvk, "canon", (1920, 1080, 0), 10000, HASH, 0, tune={key: 2.0 ** 32})
        check_invariants(v, compute(rtvk, v))


def test_row_weights_band_height_not_a_multiple_of_8(rtvk):
    """12 rows of 2 x 2 tiles with costs [10, 20 / 30, 40] and no order: the tile rows weigh 30 and 70;
    the first holds 8 band rows (30 / 8 = 3.75 each), the second the remaining 4 (70 / 4 = 17.5)."""
    w = rtvk.row_weights([10, 20, 30, 40], None, tiles_x=2, band_h=12)
    assert w.tolist() == [3.75] * 8 + [17.5] * 4


def test_row_weights_order_entry_out_of_range(rtvk):
    """16 rows of 2 x 2 tiles with costs [1, 2 / 3, 4], order [3, 9, 0, 1], 2 head ranks of 5 chunks,
    2 chunks elsewhere. Entry 9 names no tile and is skipped, so tile 2 keeps rank 0: ranks are
    tile 0 -> 2, tile 1 -> 3, tile 2 -> 0, tile 3 -> 0; the multipliers 2, 2, 5, 5; the tile rows
    1 * 2 + 2 * 2 = 6 and 3 * 5 + 4 * 5 = 35; per band row 6 / 8 = 0.75 and 35 / 8 = 4.375."""
    w = rtvk.row_weights([1, 2, 3, 4], [3, 9, 0, 1], tiles_x=2, band_h=16, head_tiles=2, head_chunks=5, chunks=2)
    assert w.tolist() == [0.75] * 8 + [4.375] * 8
    # without a head the order does not matter: every multiplier is 1 (3 / 8 and 7 / 8)
    w = rtvk.row_weights([1, 2, 3, 4], [3, 9, 0, 1], tiles_x=2, band_h=16, head_tiles=0, head_chunks=5, chunks=2)
    assert w.tolist() == [0.375] * 8 + [0.875] * 8


def test_row_weights_without_tile_columns(rtvk):
    """tiles_x = 0: no tile row exists, every one of the 5 band rows weighs 0 (and nothing is read
    out of bounds or divided by zero). A band taller than its record's tile rows: 0 past them."""
    assert rtvk.row_weights([1, 2, 3, 4], None, tiles_x=0, band_h=5).tolist() == [0.0] * 5
    assert rtvk.row_weights([8, 8], None, tiles_x=2, band_h=10).tolist() == [2.0] * 8 + [0.0] * 2
    assert rtvk.row_weights([], None, tiles_x=3, band_h=0).tolist() == []


if __name__ == "__main__":
    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "ray-tracing-gpu-vulkan_amd")]
    import rtvk as m
    m.load_library()
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", "usage: test_launch_plan.py --write COMMIT"
    fields = [n for n, _ in m.abi.LaunchPlan._fields_]
    table = {}
    for key, kw in cases().items():
        v = make_inputs(m, **kw)
        p = compute(m, v)
        table[key] = [hashlib.sha256(bytes(v)).hexdigest()[:8], p if isinstance(p, str) else [p[f] for f in fields]]
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in table.items())
    GOLDEN.write_text(f'{{"commit": {json.dumps(sys.argv[2])},\n "fields": {json.dumps(fields)},\n "cases": {{\n{rows}\n }}}}\n')
    print(f"{len(table)} plans -> {GOLDEN} ({GOLDEN.stat().st_size} bytes)")
