"""Quality of the variance-guided denoise on the CPU: the oracle's frames of the
canonical scene in the counter-based stream at 96x54, rendered as two halves, 16 feature samples,
the default parameters, through the numpy restatement (tests/denoise_var_sim.py), against the
oracle's 1024-spp frame. PSNR on sqrt(clip(mean)). Only the orderings that held at both sizes of
the prototype (96x54 and 240x135) with more than 1.5 dB to spare are asserted:
  4 spp          variance-guided above the noisy frame
  32 and 64 spp  variance-guided above the plain filter (denoise_sim.denoise on A + B)"""
import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv

W, H, F, REF_SPP = 96, 54, 16, 1024
f32 = np.float32


@pytest.fixture(scope="module")
def frames(oracle):
    sc = oracle.generate_scene()
    ref, _, _ = oracle.render(sc, oracle.render_call_info(REF_SPP, W, H), W, H, opts=oracle.options(rng_mode=ds.HASH))
    feat0, feat1 = ds.features(oracle, sc, oracle.render_call_info(REF_SPP, W, H), W, H, F)
    ref_mean = ref[..., :3] / f32(REF_SPP)

    def at(spp):
        h = spp // 2
        rci = oracle.render_call_info(h, W, H)
        A, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=0))
        B, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=h))
        noisy = ds.psnr((A + B)[..., :3] / f32(spp), ref_mean)
        plain = ds.psnr(ds.denoise(A + B, feat0, feat1, F, spp=spp), ref_mean)
        guided = ds.psnr(dv.denoise(A, B, feat0, feat1, F, half_spp=h), ref_mean)
        print(f"{W}x{H} {spp:3d} spp: noisy {noisy:.2f} dB, plain {plain:.2f} dB, variance-guided {guided:.2f} dB")
        return noisy, plain, guided
    return at


def test_at_4_spp_above_the_noisy_frame(frames):
    noisy, _, guided = frames(4)
    assert guided > noisy


@pytest.mark.parametrize("spp", [32, 64])
def test_above_the_plain_filter(frames, spp):
    _, plain, guided = frames(spp)
    assert guided > plain
