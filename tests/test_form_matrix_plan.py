"""The premise of tests/test_gpu_form_matrix.py on the CPU: every recipe of tests/form_matrix.py,
planned by the host (rtvk.launch_plan on tests/test_launch_plan.py's input model and scene
summaries), yields the kernel form it is there for, and the recipes together reach every cell of
rt_kernels.hip pick(): all 12 ACCEL_* values, the three one-layer twins and the camera-batch
kernel. A later change to choose_accel cannot hollow the matrix out unnoticed.

The summaries stand for the scenes: `canon` for the host-built canonical scene, `dev1028` for a
device-built one whose grid is walked from L2, `c5` for a device-built scene too large for any LDS
tree; a recipe on the `stack` scene takes its summary with a grid three cells thick in y."""
import pytest

import form_matrix as fm
import test_launch_plan as lp
from test_launch_plan import HASH, STREAM, rtvk  # noqa: F401  (module fixture)

BAND = (44, 27, 1)      # the GPU test's band, with a rows map
PLAIN = (44, 27, 0)


def inputs(rtvk, r, band=BAND, spp=7, stream=HASH, reserved0=0):
    more = {}
    if r.layered:
        n = lp.SCENES[r.model]["grid_n"]
        more = dict(grid_n=(n[0], 3, n[2]), grid_n_cells=3 * lp.SCENES[r.model]["grid_n_cells"])
    tune = {k: v for k, v in r.tune.items() if k != "camera_batches"}   # (kept beside the plan's tuning values)
    return lp.make_inputs(rtvk, r.model, band, spp, stream, "brute" if r.accel == fm.BRUTE else r.reserved1, tune=tune,
                          reserved0=reserved0, **more)


def planned(rtvk, v):
    """(the plan, its form's name, its one-layer answer)."""
    p = lp.compute(rtvk, v)
    assert isinstance(p, dict), p
    name = {a: n for n, a in fm.ACCEL.items()}[p["accel"]]
    return rtvk.launch_plan(v), name, bool(p["flat"])


@pytest.mark.parametrize("stream", [STREAM, HASH])
@pytest.mark.parametrize("band", [BAND, PLAIN])
@pytest.mark.parametrize("r", fm.RECIPES, ids=lambda r: r.id)
def test_recipe_yields_its_form(rtvk, r, band, stream):
    _, name, flat = planned(rtvk, inputs(rtvk, r, band=band, stream=stream))
    assert (name, flat) == (r.form, r.flat)


def test_recipes_reach_every_cell(rtvk):
    got = {planned(rtvk, inputs(rtvk, r))[1:] for r in fm.RECIPES}
    assert {name for name, _ in got} == set(fm.ACCEL) and len(fm.ACCEL) == 12
    assert {name for name, flat in got if flat} == set(fm.FLAT_TWINS)
    assert {name for name, flat in got if not flat} == set(fm.ACCEL)   # every form's general kernel too
    assert len(got) == 15 and len(fm.RECIPES) == 16   # 15 (form, one-layer) pairs and the camera-batch kernel
    assert {r.form: r.flat for r in fm.RECIPES if r.flat} == {n: True for n in fm.FLAT_TWINS}
    assert [r.id for r in fm.RECIPES if r.batch] == ["camera-batch"]
    # the scenes' sizes are what the summaries' forms assume: records for at most 512 spheres
    assert fm.N_SPHERES["canon"] <= 512 and fm.N_SPHERES["stack"] <= 512 < fm.N_SPHERES["k40"]


@pytest.mark.parametrize("r", fm.RECIPES, ids=lambda r: r.id)
def test_instrumented_launches_are_never_one_layer(rtvk, r):
    for stream in (STREAM, HASH):
        plan, name, flat = planned(rtvk, inputs(rtvk, r, stream=stream, reserved0=1))
        assert name == r.form and not flat and plan.count == 1


@pytest.mark.parametrize("r", fm.RECIPES, ids=lambda r: r.id)
def test_rows_map_offset(rtvk, r):
    """The rows map of the 44x27 band in the plan's dynamic LDS: past the form's own bytes for the LDS
    forms, at byte 0 for the L2 forms, not staged for brute force; and no plan without a rows map
    names an offset."""
    plan, name, _ = planned(rtvk, inputs(rtvk, r))
    fm.rows_lds_check(name, plan, BAND[1])
    if name == "lbvh-treelet":   # the model's two blocks per CU end at 64 KiB: 65 504 + 108 B do not fit
        assert plan.rows_lds == fm.NO_ROWS_LDS
    plain, _, _ = planned(rtvk, inputs(rtvk, r, band=PLAIN))
    assert plain.rows_lds == fm.NO_ROWS_LDS and plain.lds == plan.lds - (4 * BAND[1] if plan.rows_lds != fm.NO_ROWS_LDS else 0)


def test_camera_batch_recipe(rtvk):
    """The camera-batch recipe's plan takes the form for the HASH launch with the uniform hand-out,
    with and without a rows map, and gives the reason the GPU test asserts for every other launch
    kind; the grid-lds-rec recipe differs from it by its tuning value alone."""
    r = fm.BY_ID["camera-batch"]
    for band in (BAND, PLAIN):
        v = inputs(rtvk, r, band=band)
        lp.compute(rtvk, v)
        assert rtvk.camera_batches(v)["on"]
        assert rtvk.camera_batches(v, table=True)["why"] == "table"
        assert rtvk.camera_batches(v, tune=fm.BY_ID["grid-lds-rec-flat"].tune["camera_batches"])["why"] == "tune"
        v = inputs(rtvk, r, band=band, stream=STREAM)
        lp.compute(rtvk, v)
        assert rtvk.camera_batches(v)["why"] == "stream"
        v = inputs(rtvk, r, band=band, reserved0=1)
        lp.compute(rtvk, v)
        assert rtvk.camera_batches(v)["why"] == "count"
    for other in fm.RECIPES:   # no other recipe's plan admits the form, whatever its tuning value
        if other.batch or other.id == "grid-lds-rec-flat":
            continue
        v = inputs(rtvk, other)
        lp.compute(rtvk, v)
        assert rtvk.camera_batches(v)["why"] == "form", other.id
