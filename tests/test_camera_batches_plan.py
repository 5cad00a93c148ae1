"""The host's decision for the camera-batch form of the LDS grid kernel (csrc/rt_launch.cpp
camera_batches) on the CPU, through rt_debug_camera_batches on the inputs
tests/test_launch_plan.py builds: the form is taken for the canonical scene's hash-stream launch
with the uniform hand-out, and refused, each time for the reason stated, for the reference stream,
a table launch, an instrumented launch, the L2 grid and the other forms, a camera without
pinhole_lf, LDS bytes beyond the two-block budget, a kernel that does not reach the plan's blocks per
CU, a depth the queue's word cannot hold, and the tuning value 0. The LDS bytes it reports are the
kernel's: the static part is what the compiler reports for rt_trace_grid_batch_kernel (55 408 B:
18 432 of pixel sums, 36 864 of queue and chain counters, 112 of walk parameters), the total adds the
plan's dynamic bytes."""
import pytest

import test_launch_plan as lp
from test_launch_plan import HASH, STREAM, rtvk  # noqa: F401  (module fixture)

FULL = (1920, 1080, 0)
STATIC = 3 * 8 * 768 + (4 + 16 + 16 + 12) * 768 + 112
TWO_BLOCKS = 78 * 1024


def decide(rtvk, scene="canon", band=FULL, spp=10000, stream=HASH, form=0, tune=None, edit=None, batch_tune=-1.0,
           **how):
    v = lp.make_inputs(rtvk, scene, band, spp, stream, form, tune=tune)
    if edit:
        for k, x in edit.items():
            setattr(v, k, x)
    plan = lp.compute(rtvk, v)   # (sets the one-layer answer of the inputs)
    return rtvk.camera_batches(v, tune=batch_tune, **how), plan


def test_taken_for_the_headline_launch(rtvk):
    d, plan = decide(rtvk)
    assert plan["accel"] == lp.GRID_REC and plan["flat"] == 1 and plan["blocks_per_cu"] == 2
    assert d["on"] and d["why"] == "on"
    assert d["static_lds"] == STATIC == 55408
    assert d["lds_total"] == STATIC + plan["lds"] <= TWO_BLOCKS
    # ... with the rows map of a strip staged behind the grid, and with the kernel's own answer
    d, plan = decide(rtvk, band=(1920, 135, 1), kernel_blocks=2)
    assert plan["rows_lds"] != 0xffffffff and d["on"] and d["lds_total"] == STATIC + plan["lds"]
    assert plan["lds"] == ((plan["grid_bytes"] + 15) & ~15) + 135 * 4
    for spp in (1, 7, 100):
        assert decide(rtvk, band=(64, 36, 0), spp=spp)[0]["on"]


@pytest.mark.parametrize("why,kw", [
    ("stream", dict(stream=STREAM)),
    ("table", dict(table=True)),
    ("count", dict(edit=dict(reserved0=1))),
    ("form", dict(scene="c5", band=(3840, 2160, 0), spp=1000)),        # the grid from L2
    ("form", dict(scene="nogrid")),                                     # a tree
    ("form", dict(form="brute")),
    ("form", dict(form=16)),                                            # the candidate-queue A/B form
    ("form", dict(tune=dict(grid_rec=0))),                              # the plain LDS grid kernel
    ("form", dict(edit=dict(grid_n_refs=2500))),                        # records no longer fit: the plain LDS grid kernel
    ("form", dict(edit=dict(grid_n=(lp.CANON["grid_n"][0], 2, lp.CANON["grid_n"][2])))),   # two layers of cells
    ("pinhole", dict(edit=dict(pinhole_lf=0))),
    ("lds", dict(band=(8, 8000, 1))),                                   # a rows map of 32 000 B behind the grid
    ("occupancy", dict(kernel_blocks=1)),
    ("depth", dict(max_depth=(1 << 26) + 1)),
    ("tune", dict(batch_tune=0)),
])
def test_refused(rtvk, why, kw):
    d, plan = decide(rtvk, **kw)
    assert not d["on"] and d["why"] == why, (d, plan)
    if why == "lds":
        assert plan["accel"] == lp.GRID_REC and plan["blocks_per_cu"] == 2 and d["lds_total"] > TWO_BLOCKS


def test_tuning_value(rtvk):
    """Unset (-1) and 1 take the form, 0 does not; values outside rt_debug_tune's domain are refused."""
    assert decide(rtvk, tune=None)[0]["on"]
    v = lp.make_inputs(rtvk, "canon", FULL, 10000, HASH, 0)
    lp.compute(rtvk, v)
    assert rtvk.camera_batches(v, tune=1)["on"] and rtvk.camera_batches(v, tune=-1)["on"]
    assert rtvk.camera_batches(v, tune=0)["why"] == "tune"
    for bad in (-2.0, float("nan"), 1e30):
        with pytest.raises(rtvk.RtError):
            rtvk.camera_batches(v, tune=bad)
