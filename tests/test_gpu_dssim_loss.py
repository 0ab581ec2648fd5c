"""GPU: the exact D-SSIM loss (dssim_mode="gaussian", csrc/dssim.hip).  Its loss image against the float64 restatement (tests/dssim64.py),
exact zeros for identical images, agreement with the reference loss where lambda_dssim is 0, determinism and recording, the backward pass's
accumulators against the oracle's backward raster fed with the same loss image, and the Trainer's wiring."""
import numpy as np
import pytest

from webdgs_amd import ops, synth

import dssim64
import harness
import ssim64
from harness import assert_bits_equal
from test_gpu_eval import EDGE_SIZES, KINDS, SIZES, _pair, _trainer, _views

pytestmark = pytest.mark.gpu

LAMBDAS = [(0.8, 0.0, 0.2), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)]
REL_TOL = 2e-4


def _pass(dev, w, h, **tc):
    pc = ops.createPointCloud(dev, np.zeros((1, 6), np.uint32), np.zeros((1, 24), np.uint32), 0)
    return ops.TiledBackwardPass(dev, pc, dict(viewportWidth=w, viewportHeight=h, trainingConfig=tc))


def _lam(lam):
    return dict(lambda_l1=lam[0], lambda_l2=lam[1], lambda_dssim=lam[2])


def _loss_image(bwd, pred, targ, w, h):
    bwd.computeLossOnly(None, pred, targ)
    return bwd.getLossTextureView().read(np.float32).reshape(h, w, 4)


@pytest.mark.parametrize("w,h", SIZES + EDGE_SIZES)
def test_loss_image_matches_float64(hip_device, w, h):
    dev = hip_device
    bwd = _pass(dev, w, h, dssim_mode="gaussian")
    try:
        for k, kind in enumerate(KINDS):
            a, b = _pair(kind, w, h, seed=w * 7919 + h * 31 + k)
            ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
            x, y = ssim64.rgb01(a), ssim64.rgb01(b)
            d = x - y
            gs = None if kind == "identical" else np.moveaxis(dssim64.ssim_sum_grad(x, y), 0, -1)
            for lam in LAMBDAS:
                bwd.setTrainingConfig(_lam(lam))
                got = _loss_image(bwd, ba, bb, w, h)
                assert np.all(got[..., 3] == 1.0)
                if kind == "identical":
                    assert np.all(got[..., :3] == 0.0), f"{w}x{h} {lam}: identical images must give exactly 0"
                    continue
                want = lam[0] * np.sign(np.moveaxis(d, 0, -1)) + lam[1] * np.moveaxis(d, 0, -1) - lam[2] * gs
                err = np.abs(got[..., :3] - want) / np.maximum(1.0, np.abs(want))
                worst = float(err.max())
                print(f"dssim loss {w}x{h} {kind} {lam}: max |g - g64| / max(1, |g64|) = {worst:.3e}, max |g64| = {float(np.abs(want).max()):.3e}")
                assert worst <= REL_TOL, f"{w}x{h} {kind} {lam}: off by {worst}"
    finally:
        bwd.destroy()


def test_lambda_dssim_zero_equals_reference_mode(hip_device):
    dev = hip_device
    w, h = 203, 117
    a, b = _pair("noise", w, h, seed=3)
    ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
    ref = _pass(dev, w, h, lambda_l1=0.7, lambda_l2=0.4, lambda_dssim=0.0)
    gau = _pass(dev, w, h, lambda_l1=0.7, lambda_l2=0.4, lambda_dssim=0.0, dssim_mode="gaussian")
    try:
        assert_bits_equal(_loss_image(gau, ba, bb, w, h), _loss_image(ref, ba, bb, w, h), "lambda_dssim = 0: gaussian vs reference")
        # a pass switched to gaussian and back gives the reference bits again
        ref.setTrainingConfig(dict(lambda_dssim=0.2))
        today = _loss_image(ref, ba, bb, w, h).copy()
        ref.setTrainingConfig(dict(dssim_mode="gaussian"))
        g = _loss_image(ref, ba, bb, w, h).copy()
        assert not np.array_equal(g, today)
        ref.setTrainingConfig(dict(dssim_mode="reference"))
        assert_bits_equal(_loss_image(ref, ba, bb, w, h), today, "gaussian and back")
        fresh = _pass(dev, w, h, lambda_l1=0.7, lambda_l2=0.4, lambda_dssim=0.2)
        assert_bits_equal(_loss_image(fresh, ba, bb, w, h), today, "a fresh reference pass")
        fresh.destroy()
    finally:
        ref.destroy()
        gau.destroy()


def test_deterministic_and_recordable(hip_device):
    dev = hip_device
    w, h = 1920, 1080
    a, b = _pair("smooth", w, h, seed=9)
    ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
    bwd = _pass(dev, w, h, dssim_mode="gaussian")
    try:
        first = _loss_image(bwd, ba, bb, w, h).copy()
        for _ in range(3):
            assert_bits_equal(_loss_image(bwd, ba, bb, w, h), first, "repeated computeLossOnly")
        with dev.createCommandEncoder("dssim loss", record=True) as enc:
            bwd.computeLossOnly(enc, ba, bb)
            cmd = enc.finish()
        bwd.getLossTextureView().clear()
        dev.queue.submit([cmd])
        dev.queue.submit([cmd])
        assert_bits_equal(bwd.getLossTextureView().read(np.float32).reshape(h, w, 4), first, "replayed recording")
        # the recording keeps the mode it was recorded with
        bwd.setTrainingConfig(dict(dssim_mode="reference"))
        bwd.getLossTextureView().clear()
        dev.queue.submit([cmd])
        assert_bits_equal(bwd.getLossTextureView().read(np.float32).reshape(h, w, 4), first, "replay after a mode change")
        cmd.destroy()
    finally:
        bwd.destroy()


def test_backward_accumulators_equal_the_oracle(hip_device, orc):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20000, width=320, height=240, sh_deg=1, s0=0.02)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8)[3]
    tg, tsh = synth.make_target_scene(g, sh)
    tp = harness.HipPipeline(dev, cfg, tg, tsh, cam)
    tp.forward()
    target = dev.bufferFrom(tp.rast.getOutputTextureView().read(np.uint8))
    tp.destroy()
    n = cfg.num_points
    tc = dict(dssim_mode="gaussian")

    def run(pipe):
        pipe.forward()
        pipe.bwd.encode(None, pipe.rast.getOutputTextureView(), target, pipe.backward_resources(), None)
        dev.synchronize()
        return (pipe.bwd.getAccumulatorsBuffer().read(np.int32).copy(), pipe.bwd.getGradientsBuffer().read(np.uint32).copy(),
                pipe.bwd.getLossTextureView().read(np.float32).reshape(cfg.height, cfg.width, 4).copy())

    p1 = harness.HipPipeline(dev, cfg, g, sh, cam, training_config=tc)
    p2 = harness.HipPipeline(dev, cfg, g, sh, cam, training_config=tc)
    try:
        acc_a, grad_a, loss_a = run(p1)
        acc_b, grad_b, _ = run(p1)       # the second encode of one pass: the accumulators were cleared in between
        acc_f, grad_f, _ = run(p2)
        assert np.any(acc_a != 0)
        assert_bits_equal(acc_b, acc_f, "second encode vs a fresh pass: accumulators")
        assert_bits_equal(grad_b, grad_f, "second encode vs a fresh pass: packed gradients")
        assert_bits_equal(acc_a, acc_f, "first encode vs a fresh pass: accumulators")
        # the accumulators are the oracle's backward raster of the GPU's own loss image
        fw = p1.collect_forward()
        bs = synth.render_settings(cfg).copy()
        bs[5] = 0.0
        gm, gc, go, gcol = orc.backward_rasterize(bs, n, fw["tile_ranges"], fw["sorted_values"], fw["splats"], fw["final_T"], fw["n_contrib"], loss_a)
        hm, hc, ho, hcol = harness.acc_to_reference_layout(acc_b, n)
        assert_bits_equal(hm, gm, "mean accumulators")
        assert_bits_equal(hc, gc, "conic accumulators")
        assert_bits_equal(ho, go, "opacity accumulators")
        assert_bits_equal(hcol, gcol, "colour accumulators")
        # and the gaussian loss is a different loss: the reference mode's accumulators differ
        p1.bwd.setTrainingConfig(dict(dssim_mode="reference"))
        acc_r, _, _ = run(p1)
        assert not np.array_equal(acc_r, acc_b)
    finally:
        p1.destroy()
        p2.destroy()


def _run_trainer(dev, cfg, g, sh, cameras, images, steps=13, **kw):
    t = _trainer(dev, cfg, g, sh, cameras, images, **kw)
    for _ in range(steps):
        t.step()
    t.drain()
    st = t.optimizer.getStateBuffers()
    out = dict(n=t.getPointCount(), g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32),
               **{k: st[k].read(np.uint32) for k in st})
    t.destroy()
    return out


@pytest.mark.parametrize("pipeline_depth,views_per_rank", [(1, 1), (2, 1), (1, 8), (2, 8)])
def test_trainer_runs_are_bit_equal(hip_device, pipeline_depth, views_per_rank):
    """13 steps across two densify events in gaussian mode, twice: cloud, SH rows and the six optimizer state arrays equal bit for bit;
    at 8 views per rank one lane gives the default lanes' bits; the reference mode trains something else."""
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 8)
    kw = dict(pipeline_depth=pipeline_depth, views_per_rank=views_per_rank, trainingConfig=dict(dssim_mode="gaussian"))
    runs = [_run_trainer(dev, cfg, g, sh, cameras, images, **kw) for _ in range(2)]
    if views_per_rank > 1:
        runs.append(_run_trainer(dev, cfg, g, sh, cameras, images, overlap_views=False, **kw))
    assert runs[0]["n"] != 5000, "the run crosses densify rebuilds"
    for r in runs[1:]:
        assert r["n"] == runs[0]["n"]
        for k in runs[0]:
            if k != "n":
                assert_bits_equal(r[k], runs[0][k], f"gaussian-mode runs: {k}")
    if (pipeline_depth, views_per_rank) == (1, 1):
        ref = _run_trainer(dev, cfg, g, sh, cameras, images, pipeline_depth=1, views_per_rank=1)
        assert ref["n"] != runs[0]["n"] or not np.array_equal(ref["g"], runs[0]["g"])


def test_trainer_set_training_config_reaches_the_backward_pass(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, images, densify=False)
    check = _pass(dev, cfg.width, cfg.height, dssim_mode="gaussian")
    try:
        for _ in range(3):
            t.step()
        for k, mode in [(2, "gaussian"), (1, "reference"), (3, "gaussian")]:
            t.setTrainingConfig(dict(dssim_mode=mode))
            assert t.getTrainingConfig()["dssim_mode"] == mode
            t.step(view_ids=[k])
            t.drain()
            pred = dev.bufferFrom(t.rasterizer.getOutputTextureView().read(np.uint8))
            check.setTrainingConfig(dict(dssim_mode=mode))
            want = _loss_image(check, pred, images[k]["texture"], cfg.width, cfg.height)
            assert_bits_equal(t.backwardPass.getLossTextureView().read(np.float32).reshape(cfg.height, cfg.width, 4), want, f"step on view {k}, {mode}")
        with pytest.raises(ValueError):
            t.setTrainingConfig(dict(dssim_mode="box"))
        assert t.getTrainingConfig()["dssim_mode"] == "gaussian"
    finally:
        check.destroy()
        t.destroy()


def test_held_out_psnr_and_ssim_rise_over_training(hip_device):
    """The setting of test_gpu_eval.test_held_out_psnr_and_ssim_rise_over_training, trained on the exact D-SSIM loss; both modes' numbers are
    printed (DESIGN.md section 9 quotes them)."""
    from webdgs_amd import loaders
    dev = hip_device
    cfg = harness.small_config("c2", num_points=4000, width=160, height=128, sh_deg=0, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 24)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images)
    tg, tsh = synth.make_target_scene(g, sh)
    h16 = tsh.copy().view(np.uint16).reshape(-1, 48)
    dc = h16[:, 0:3].view(np.float16).astype(np.float32) + np.random.default_rng(7).normal(0.0, 0.5, (len(h16), 3)).astype(np.float32)
    h16[:, 0:3] = synth.f32_to_f16_bits(dc)
    res = {}
    for mode in ("gaussian", "reference"):
        t = _trainer(dev, cfg, tg, h16.view(np.uint32).reshape(-1, 24), trc, tri, seed=11, densify=False, trainingConfig=dict(dssim_mode=mode))
        t.setOptimizerHyperparameters(dict(lr_pos=0.0, lr_rot=0.0, lr_scale=0.0))
        t.setEvaluationViews(tec, tei)
        r0 = t.evaluate()
        for _ in range(200):
            t.step()
        r1 = t.evaluate()
        t.destroy()
        res[mode] = (r0, r1)
        print(f"held-out, {mode} loss: PSNR {r0['mean_psnr']:.3f} -> {r1['mean_psnr']:.3f} dB, SSIM {r0['mean_ssim']:.5f} -> {r1['mean_ssim']:.5f}")
    r0, r1 = res["gaussian"]
    assert r1["mean_psnr"] > r0["mean_psnr"] + 0.5
    assert r1["mean_ssim"] > r0["mean_ssim"]
