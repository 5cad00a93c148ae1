"""Every trace-kernel form in every launch kind against the oracle (DESIGN.md §4.3's matrix).

rt_kernels.hip pick() turns a launch into one template instantiation out of forms x launch kinds;
each cell is a kernel of its own (its registers, and the planned launches stage the rows map at a
form-specific LDS offset). tests/form_matrix.py holds one recipe per form, the kinds are:

  stream      RT_RNG_PIXEL_STREAM, 3 spp, against oracle.render
  hash-rows   HASH, 7 spp from sample_base 1000 through a non-monotonic rows map
              (test_sample_map.ROWS: 19 rows of a 44x40 image), accumulated onto a non-zero
              accumulator; the plan's rows_lds is the form's (form_matrix.rows_lds_check)
  levels      a sample-map frame of EXAMPLE under the level schedule (the tile lists)
  one-launch  the same table under RT_SAMPLE_MAP_ONE_LAUNCH at unit 3 (a host block table), at the
              default refill_reserve and at 0, so both hand-out phases read the table
  feedback    two chained feedback frames from START at unit 5 (a device block table): the frames,
              the next counts, (E, S) and the device's tables
  adaptive    one adaptive frame (the passes' tile lists): image, counts, passes, samples
  count       the instrumented kernels, STREAM and HASH with the uniform hand-out

Every band is 44x27 (6 x 4 tiles, ragged both ways; 44x19 under the rows map). The standard of proof
is the suite's: every accumulator float, every rgba8 byte and every per-texel count equal, the outputs
pre-filled with sentinels. After its launches every case asserts launch_info()'s form, flat_grid and
camera_batches against the recipe, so a fall-back to another form fails instead of passing.

The camera-batch kernel runs only rt_render_device's HASH launches with the uniform hand-out (with and
without a rows map: its hash-rows case); in every other kind its recipe runs the one-layer
grid-lds-rec kernel and the case asserts the reason rt_debug_camera_batches gives for that launch.

References depend on (scene, kind) only and are computed once (adaptive_sim's caches, and lru_cache
here). The adaptive thresholds were chosen on the CPU simulation so that adaptive_sim.assert_not_vacuous
holds: canon 0.2 {16: 1, 24: 1, 32: 4, 40: 5, 48: 2, 56: 5, 64: 6}, stack 0.15 {24: 1, 32: 2, 40: 1,
48: 3, 56: 3, 64: 14}, k40 0.2 {8: 1, 24: 1, 32: 4, 40: 2, 48: 5, 56: 4, 64: 7}."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
import form_matrix as fm   # noqa: E402
from test_gpu_parity import assert_same, tree_builder, tuned   # noqa: E402
from test_sample_map import EXAMPLE, ROWS, adaptive_parity, lib, map_parity, torch   # noqa: E402,F401  (module fixtures)
from test_sample_map_feedback import START, chain   # noqa: E402
from test_sample_map_one_launch import one_launch_parity   # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 44, 27
IMAGE = (44, 40)   # the image ROWS indexes
KINDS = ["stream", "hash-rows", "levels", "one-launch", "feedback", "adaptive", "count"]
ADAPTIVE_THR = {"canon": 0.2, "stack": 0.15, "k40": 0.2}
# why the camera-batch recipe's launch of a kind is not the camera-batch kernel (rtvk.CAMERA_BATCH_REASONS;
# table: not the uniform hand-out)
BATCH_OFF = {"stream": "stream", "levels": "table", "one-launch": "table", "feedback": "table", "adaptive": "table"}
CASES = [(r, kind) for r in fm.RECIPES for kind in KINDS]


class Bench:
    """One renderer for the module; the scene is set again only when a case needs another."""

    def __init__(self, lib):
        self.r = lib.Renderer(0)
        self.held = None

    def use(self, oracle, recipe):
        key = (recipe.scene, recipe.builder)
        if key != self.held:
            self.held = None
            with tree_builder(recipe.builder):
                self.r.set_scene(np.ascontiguousarray(fm.scene(oracle, recipe.scene)))
            self.held = key
        about = self.r.scene_array(8)
        assert about["n_spheres"] == fm.N_SPHERES[recipe.scene] and about["device_built"] == (recipe.builder == "gpu")
        assert (self.r.scene_array(9)["n"][1] == 1) == (recipe.scene != "stack")   # the grid's thickness in y
        return self.r


@pytest.fixture(scope="module")
def bench(lib, torch):
    b = Bench(lib)
    yield b
    b.r.close()


def sim_key(oracle, scene):
    """The scene's key in adaptive_sim."""
    return 11 if scene == "canon" else sim.register(scene, fm.scene(oracle, scene))


@functools.lru_cache(maxsize=None)
def uniform_ref(oracle, scene, rng, spp):
    ra, ro, st = oracle.render(fm.scene(oracle, scene), oracle.render_call_info(spp, W, H), W, H,
                               opts=oracle.options(rng_mode=rng), threads=16)
    return ra, ro, st[:2]


@functools.lru_cache(maxsize=None)
def rows_ref(oracle, scene):
    """(the accumulator the frame adds to: 2 samples; the frame on top of it: 7 from sample 1000)."""
    sc, h = fm.scene(oracle, scene), len(ROWS)
    a0, _, _ = oracle.render(sc, oracle.render_call_info(2, *IMAGE), W, h, rows=ROWS, opts=oracle.options(rng_mode=fm.HASH),
                             threads=16)
    ra, ro, st = oracle.render(sc, oracle.render_call_info(7, *IMAGE), W, h, rows=ROWS, accum=a0, threads=16,
                               opts=oracle.options(rng_mode=fm.HASH, accumulate=1, sample_base=1000))
    assert float(np.abs(a0[..., :3]).sum()) > 0
    return a0, ra, ro, st[:2]


def frame(lib, torch, oracle, renderer, opt, spp, h=H, image=(W, H), rows=None, accum=None):
    """One rt_render_device frame: (accumulator, rgba8, stats), the outputs pre-filled with sentinels
    (the accumulator with `accum` where the frame adds to one)."""
    rci = lib.RenderCallInfo.from_buffer_copy(oracle.render_call_info(spp, *image).tobytes())
    acc = (torch.full((h, W, 4), -1.0, dtype=torch.float32, device="cuda") if accum is None
           else torch.from_numpy(np.ascontiguousarray(accum, np.float32)).cuda())
    out = torch.full((h, W, 4), 7, dtype=torch.uint8, device="cuda")
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    renderer.render_device(rci, acc, out, rows=rows_t, options=opt)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), out.cpu().numpy(), renderer.stats()


def check_launch(lib, renderer, recipe, batch=False, count=False, why=None):
    """launch_info() of the last launch against the recipe: the form, the one-layer answer (never for
    an instrumented launch), the camera-batch kernel; `why`: the reason the plan gives against it."""
    info = renderer.launch_info()
    what = (recipe.id, info)
    assert info["form"] == recipe.form, what
    assert info["flat_grid"] == (recipe.flat and not count), what
    assert info["camera_batches"] == batch, what
    inputs, plan = renderer.launch_plan()
    assert plan.accel == fm.ACCEL[recipe.form] and plan.count == int(count), what
    assert inputs.reserved1 == recipe.reserved1 and inputs.n_spheres == fm.N_SPHERES[recipe.scene], what
    if why is not None:
        tune = recipe.tune.get("camera_batches", -1.0)
        got = lib.camera_batches(inputs, tune=tune, max_depth=50, table=why == "table")
        assert not got["on"] and got["why"] == why, (what, got)
    return inputs, plan


@pytest.mark.parametrize("recipe,kind", CASES, ids=[f"{r.id}-{kind}" for r, kind in CASES])
def test_form_in_launch_kind(lib, torch, oracle, bench, recipe, kind):
    renderer = bench.use(oracle, recipe)
    key = sim_key(oracle, recipe.scene)
    opt = fm.options(lib, recipe)
    off = BATCH_OFF.get(kind) if recipe.batch else None
    with tuned(renderer, **recipe.tune):
        if kind == "stream":
            ra, ro, rst = uniform_ref(oracle, recipe.scene, fm.STREAM, 3)
            a, o, st = frame(lib, torch, oracle, renderer, fm.options(lib, recipe, rng_mode=fm.STREAM), 3)
            check_launch(lib, renderer, recipe, why=off)
            assert_same(a, o, ra, ro)
            assert (st.segments, st.samples) == rst
        elif kind == "hash-rows":
            a0, ra, ro, rst = rows_ref(oracle, recipe.scene)
            a, o, st = frame(lib, torch, oracle, renderer,
                             fm.options(lib, recipe, rng_mode=fm.HASH, accumulate=True, sample_base=1000), 7, h=len(ROWS),
                             image=IMAGE, rows=ROWS, accum=a0)
            inputs, plan = check_launch(lib, renderer, recipe, batch=recipe.batch)
            assert inputs.has_rows == 1 and (inputs.band_w, inputs.band_h) == (W, len(ROWS))
            fm.rows_lds_check(recipe.form, plan, len(ROWS))
            assert_same(a, o, ra, ro)
            assert (st.segments, st.samples) == rst
            if recipe.batch:   # ... and without a rows map
                ra, ro, rst = uniform_ref(oracle, recipe.scene, fm.HASH, 3)
                a, o, st = frame(lib, torch, oracle, renderer, fm.options(lib, recipe, rng_mode=fm.HASH), 3)
                _, plan = check_launch(lib, renderer, recipe, batch=True)
                assert plan.rows_lds == fm.NO_ROWS_LDS
                assert_same(a, o, ra, ro)
                assert (st.segments, st.samples) == rst
        elif kind == "levels":
            map_parity(lib, renderer, torch, oracle, W, H, EXAMPLE, k=key, set_scene=False, options=opt)
            check_launch(lib, renderer, recipe, why=off)
        elif kind == "one-launch":
            for reserve in (None, 0):   # the default: the last 8 192 units one by one; 0: every unit by blocks
                with tuned(renderer, refill_reserve=reserve):
                    one_launch_parity(lib, renderer, torch, oracle, W, H, EXAMPLE, unit=3, k=key, set_scene=False,
                                      options=opt)
                    check_launch(lib, renderer, recipe, why=off)
        elif kind == "feedback":
            tables = chain(lib, renderer, torch, oracle, 2, unit=5, k=key, set_scene=False, options=opt)
            assert tables[1] != tables[0]
            check_launch(lib, renderer, recipe, why=off)
        elif kind == "adaptive":
            adaptive_parity(lib, renderer, torch, oracle, W, H, k=key, thr=ADAPTIVE_THR[recipe.scene], options=opt)
            check_launch(lib, renderer, recipe, why=off)
        else:
            assert kind == "count"
            for rng in (fm.STREAM, fm.HASH):
                ra, ro, rst = uniform_ref(oracle, recipe.scene, rng, 3)
                a, o, st = frame(lib, torch, oracle, renderer, fm.options(lib, recipe, rng_mode=rng, count_tests=True), 3)
                check_launch(lib, renderer, recipe, count=True,
                             why=("stream" if rng == fm.STREAM else "count") if recipe.batch else None)
                assert_same(a, o, ra, ro)
                assert (st.segments, st.samples) == rst
                assert st.sphere_tests > 0
                if recipe.form in fm.TREE_FORMS:
                    assert st.box_tests > 0


def test_the_matrix_is_whole():
    """15 (form, one-layer) pairs and the camera-batch kernel, each in every kind: nothing left out."""
    assert len({(r.form, r.flat) for r in fm.RECIPES}) == 15 and sum(r.batch for r in fm.RECIPES) == 1
    assert len(CASES) == 16 * len(KINDS) == len(set((r.id, kind) for r, kind in CASES))
