"""The halves of feedback frames through the filters on the GPU: frames
of a camera that steps 0.05 between them hand accum_a, accum_b and half_count to the reprojected
temporal call (sample_count = half_count) and its outputs to the variance-guided filter (half_spp = 1);
a second branch filters the halves directly (half_count = half_count). Every plane and the rgba8 are
compared bit for bit with motion_sim, temporal_reproject_sim and denoise_var_sim, fed from
halves_sim's planes of the same frames (the features are the GPU's own, as in
test_gpu_temporal_reproject.py's real chain). The start table holds a zero tile, so h == 0 goes through
both consumers. gpu_chain is also the Python chain the command-line loop is compared with
(test_cli_feedback_denoise.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim            # noqa: E402
import denoise_var_sim as dv          # noqa: E402
import halves_sim as hs               # noqa: E402
import motion_sim as ms               # noqa: E402
import temporal_reproject_sim as tr   # noqa: E402
from test_gpu_temporal_reproject import same_bits        # noqa: E402
from test_motion_host import moved_camera                 # noqa: E402
from test_sample_map_feedback import START, step          # noqa: E402

HASH = 2
W, H = 44, 27
F, N, STEP_S = 16, 8, 0.05
THR, LO, CAP = 0.3, 4, 64
ZERO_TILE = 5
TABLE = [0 if t == ZERO_TILE else n for t, n in enumerate(START)]


def gpu_chain(rtvk, torch, oracle, frames, start=None, temporal=True, reproject=True, s=STEP_S, thr=THR, lo=LO, step_spp=LO,
              cap=CAP, feature_samples=F, history=N, direct=False, w=W, h=H):
    """`frames` frames of the feedback loop through the filters, everything queued on one stream: frame
    k at sample_base k x cap from frame k of the camera path. start: a tile table, every frame is a
    feedback halves frame from it; None: frame 0 is an adaptive halves frame (thr, lo, step_spp) and the
    map is set from it, as the command-line loop does. Then the features at sample_base 0, with
    `reproject` the motion pass and keep_current, with `temporal` the stage on the halves (sample_count
    = half_count) and the variance filter on its outputs at half_spp 1, else the filter on the halves
    with half_count; direct: that second form as well, into planes of its own. Returns per frame a dict
    of numpy planes."""
    z = lambda dtype, c=4: torch.zeros((h, w, c), dtype=dtype, device="cuda")
    acc, acc_a, acc_b, f0, f1, mv, out_a, out_b, mean, mean2 = (z(torch.float32) for _ in range(10))
    out, scratch, out2 = z(torch.uint8), z(torch.uint8), z(torch.uint8)
    half = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hlen = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    fb = rtvk.make_feedback(thr, lo, cap)
    tparams = rtvk.make_temporal(max_history=history)
    st = torch.cuda.Stream()
    res = []
    torch.cuda.synchronize()
    with rtvk.Renderer(0) as r, torch.cuda.stream(st):
        smap = r.sample_map(w, h)
        smap.schedule(rtvk.abi.SAMPLE_MAP_ONE_LAUNCH)
        T = r.temporal(w, h) if temporal else None
        M = r.motion(w, h) if reproject else None
        if start is not None:
            smap.set(torch.from_numpy(np.asarray(start, np.int32)).cuda(), stream=st)
        for k in range(frames):
            rci_np = moved_camera(oracle, cap, w, h, s, k) if s else oracle.render_call_info(cap, w, h)
            rci = rtvk.RenderCallInfo.from_buffer_copy(rci_np.tobytes())
            r.set_scene(oracle.generate_scene(0.0), stream=st)
            opt = rtvk.make_options(rng_mode=HASH, sample_base=k * cap)
            if start is None and k == 0:
                r.render_adaptive(rci, acc, scratch, options=opt, adaptive=rtvk.make_adaptive(thr, lo, step_spp), stream=st,
                                  accum_a=acc_a, accum_b=acc_b, half_count=half)
            else:
                if start is None and k == 1:
                    smap.set_from_adaptive(stream=st)
                r.render_sample_map_feedback(rci, acc, scratch, smap, fb, options=opt, stream=st, accum_a=acc_a, accum_b=acc_b,
                                             half_count=half)
            r.render_features(rci, f0, f1, samples=feature_samples, stream=st)
            if reproject:
                r.render_motion(M, rci, mv, stream=st)
                M.keep_current(rci, stream=st)
                r.temporal_reproject(T, acc_a, f0, f1, feature_samples, mv, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen,
                                     sample_count=half, params=tparams, stream=st)
            elif temporal:
                r.temporal_accumulate(T, acc_a, f0, f1, feature_samples, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen,
                                      sample_count=half, params=tparams, stream=st)
            if temporal:
                r.denoise_variance(out_a, out_b, f0, f1, feature_samples, out, half_spp=1, out_mean=mean, stream=st)
            if direct or not temporal:
                r.denoise_variance(acc_a, acc_b, f0, f1, feature_samples, out if not temporal else out2, half_count=half,
                                   out_mean=mean if not temporal else mean2, stream=st)
            st.synchronize()
            planes = dict(acc=acc, acc_a=acc_a, acc_b=acc_b, half=half, f0=f0, f1=f1, mv=mv, out_a=out_a, out_b=out_b,
                          mean=mean, out=out, hlen=hlen, mean2=mean2, out2=out2)
            res.append({name: t.cpu().numpy() for name, t in planes.items()})
            res[-1]["rci"] = rci_np
        for obj in (T, M, smap):
            if obj is not None:
                obj.close()
    return res


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rtvk(torch):
    import rtvk as m
    return m


@pytest.mark.gpu
def test_two_feedback_frames_through_both_consumers(rtvk, torch, oracle):
    frames = 2
    scene = oracle.generate_scene(0.0)
    thr_q = rtvk.threshold_q16(THR)
    res = gpu_chain(rtvk, torch, oracle, frames, start=TABLE, direct=True)
    state = tr.State(H, W)
    table, prev = hs.even_table(TABLE), None
    for k, g in enumerate(res):
        assert table[ZERO_TILE] == 0 and len({n for n in table if n}) >= 2, table
        Q = hs.cube_of(oracle, scene, g["rci"], W, H, k * CAP, max(table))
        A, B, half = hs.feedback_halves(Q, table)
        assert (half == 0).any()
        same_bits(g["acc_a"], A, (k, "accum_a"))
        same_bits(g["acc_b"], B, (k, "accum_b"))
        np.testing.assert_array_equal(g["half"].astype(np.uint32), half)
        want_mv = ms.motion(oracle, scene, g["rci"], W, H, *(prev or (None, None)))
        same_bits(g["mv"], want_mv, (k, "motion"))
        prev = (scene, g["rci"])
        # the temporal stage on the halves, then the filter on what it wrote
        w_a, w_b, _, w_n = tr.reproject(state, A, g["f0"], g["f1"], F, want_mv, accum_b=B, sample_count=half,
                                        params=(N, 4.0, 16.0))
        w_mean = dv.denoise(w_a, w_b, g["f0"], g["f1"], F, half_spp=1)
        assert np.isfinite(w_mean).all()
        same_bits(g["out_a"], w_a, (k, "out_a"))
        same_bits(g["out_b"], w_b, (k, "out_b"))
        np.testing.assert_array_equal(g["hlen"].astype(np.uint32), w_n)
        same_bits(g["mean"], w_mean, (k, "mean"))
        np.testing.assert_array_equal(g["out"], oracle.resolve(w_mean, 1))
        # the filter on the halves themselves
        d_mean = dv.denoise(A, B, g["f0"], g["f1"], F, half_count=half)
        assert np.isfinite(d_mean).all()
        same_bits(g["mean2"], d_mean, (k, "direct mean"))
        np.testing.assert_array_equal(g["out2"], oracle.resolve(d_mean, 1))
        table, _ = step(Q, table, thr_q, LO, CAP)
    # the zero tile has no measurement in either frame: texels without any history are left, beside
    # histories of two frames that followed the camera, which did move
    assert (res[1]["hlen"] == 0).any() and (res[1]["hlen"] == 2).any()
    assert np.all(res[0]["acc_a"][res[0]["half"] == 0] == np.float32([0, 0, 0, 1]))
    assert np.abs(res[1]["mv"][..., 0] - (np.arange(W) + 0.5)[None, :]).max() > 2.0 ** -6   # past the snap
