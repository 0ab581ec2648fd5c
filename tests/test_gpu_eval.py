"""GPU: held-out evaluation.  The SSIM kernel (csrc/ssim.hip) against the float64 restatement (tests/ssim64.py), its determinism, and
Trainer.evaluate: equal to a separate render + score of the flushed cloud, invisible to the training trajectory, correct for eval views of
another size and for views that overflow their tile-entry lists, and rising on held-out views while a synthetic scene trains."""
import warnings

import numpy as np
import pytest

from webdgs_amd import loaders, ops, synth
from webdgs_amd.trainer import Trainer

import harness
import ssim64
from harness import assert_bits_equal

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (10, 11), (33, 17), (160, 96), (1920, 1080), (3840, 2160)]
# Image edges against the 32x32 tiles of ssim.hip and dssim.hip and the window's radius of 5: 32x33 a second tile row of one image row (three of a
# thread's four vertical outputs outside the image); 37x38 a second tile column and row of 5 and 6 pixels (the edge at and just past the radius
# inside the D-SSIM map region's halo); 65x43 a third tile column one pixel wide and a second tile row of exactly 11 rows, one full window.
EDGE_SIZES = [(32, 33), (37, 38), (65, 43)]
KINDS = ["noise", "smooth", "flat", "identical"]


def _pair(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        a, b = rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([127 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0 - c) for c in range(3)] + [np.full_like(xx, 255)], -1)
        a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
        b = np.clip(a.astype(np.int32) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)
    elif kind == "flat":
        a = np.full((h, w, 4), 255, np.uint8)
        b = (255 - rng.integers(0, 2, (h, w, 4))).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        b = a.copy()
    return a, b


@pytest.mark.parametrize("w,h", SIZES + EDGE_SIZES)
def test_image_ssim_matches_float64(hip_device, w, h):
    dev = hip_device
    for k, kind in enumerate(KINDS):
        a, b = _pair(kind, w, h, seed=w * 7919 + h * 31 + k)
        ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
        mbuf = dev.createBuffer(12 * w * h, "ssim map")
        got = ops.imageSSIM(dev, ba, bb, w, h, mbuf)
        gmap = mbuf.read(np.float32).reshape(h, w, 3)
        if kind == "identical":
            assert got == 1.0 and np.all(gmap == 1.0), f"{w}x{h}: identical images must give exactly 1"
            continue
        want_map = ssim64.ssim_map(a, b)
        dmap, dmean = float(np.max(np.abs(gmap - want_map))), abs(got - float(want_map.mean()))
        print(f"ssim {w}x{h} {kind}: max |map - f64| = {dmap:.3e}, |mean - f64| = {dmean:.3e}")
        assert dmap <= 2e-4, f"{w}x{h} {kind}: map off by {dmap}"
        assert dmean <= 1e-6, f"{w}x{h} {kind}: mean off by {dmean}"
        # symmetric bit for bit (the shift and every operation are symmetric in a and b)
        assert ops.imageSSIM(dev, bb, ba, w, h) == got


def test_image_ssim_is_deterministic(hip_device):
    dev = hip_device
    w, h = 1920, 1080
    a, b = _pair("smooth", w, h, seed=4)
    ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
    mbuf = dev.createBuffer(12 * w * h)
    vals = [ops.imageSSIM(dev, ba, bb, w, h, mbuf if i % 2 else None) for i in range(6)]
    bits = {np.float64(v).view(np.uint64).item() for v in vals}
    assert len(bits) == 1, vals
    m1 = mbuf.read(np.uint32)
    ops.imageSSIM(dev, ba, bb, w, h, mbuf)
    assert np.array_equal(mbuf.read(np.uint32), m1)


def test_image_ssim_rejects_empty(hip_device):
    b = hip_device.createBuffer(16)
    with pytest.raises(Exception):
        ops.imageSSIM(hip_device, b, b, 0, 4)


# ----------------------------------------------------------------------------- Trainer.evaluate
def _views(dev, cfg, n_views, width=None, height=None, radius=1.0):
    """n rendered views of the target scene (cameras on a circle), at width x height (default: the config's)."""
    w, h = width or cfg.width, height or cfg.height
    vcfg = synth.SceneConfig(cfg.config_id, cfg.num_points, w, h, cfg.sh_deg, cfg.fy, cfg.s0, cfg.name)
    g, sh = synth.make_gaussians(cfg)
    tg, tsh = synth.make_target_scene(g, sh)
    cams = synth.circle_cameras(vcfg, n_views, radius=radius)
    tp = harness.HipPipeline(dev, vcfg, tg, tsh, cams[0])
    cameras, images = [], []
    for i in range(n_views):
        tp.camera.write(cams[i])
        tp.forward()
        images.append(dict(texture=dev.bufferFrom(tp.rast.getOutputTextureView().read(np.uint8)), width=w, height=h))
        cameras.append(dict(camera=cams[i], width=w, height=h))
    tp.destroy()
    return g, sh, cameras, images


def _trainer(dev, cfg, g, sh, cameras, images, seed=5, densify=True, **kw):
    t = Trainer(dev, seed=seed, **kw)
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset(cameras, images)
    if densify:
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=True, warmupIterations=6, interval=5, stopIterations=100), metricViews=2, cloneThresholdCount=2,
                                     maxNewPointsPerStep=300))
    else:
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
    t.start()
    return t


def _separate_measurement(dev, t, cameras, images):
    """A fresh TiledForwardPass + TiledRasterizer render of the flushed cloud, scored with imageSSE / imageSSIM."""
    t.flushPointCloud()
    out = []
    for c, im in zip(cameras, images):
        w, h = im["width"], im["height"]
        cam = dev.bufferFrom(np.asarray(c["camera"], np.float32))
        fw = ops.TiledForwardPass(dev, t.pointCloud, cam, dict(viewportWidth=w, viewportHeight=h, renderMode="gaussian"))
        rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fw, format="rgba8unorm"))
        fw.encode(None)
        rast.encode(None, w, h)
        pred = rast.getOutputTextureView()
        out.append((ops.imageSSE(dev, pred, im["texture"], w * h), ops.imageSSIM(dev, pred, im["texture"], w, h)))
        rast.destroy()
        fw.destroy()
    return out


def test_evaluate_equals_a_separate_measurement(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 10)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images, every=4)
    t = _trainer(dev, cfg, g, sh, trc, tri)
    assert t.deferred_sh
    t.setEvaluationViews(tec, tei)
    for _ in range(9):
        t.step()
    r = t.evaluate()
    assert r["iteration"] == 9 and r["views"] == list(range(len(tec)))
    sep = _separate_measurement(dev, t, tec, tei)
    for i, (sse, s) in enumerate(sep):
        assert r["sse"][i] == sse, f"view {i}: SSE {r['sse'][i]} vs {sse}"
        assert r["ssim"][i] == s, f"view {i}: SSIM {r['ssim'][i]!r} vs {s!r}"
        assert r["psnr"][i] == ops.psnrFromSSE(sse, cfg.width * cfg.height)
    assert r["mean_psnr"] == float(np.mean(r["psnr"])) and r["mean_ssim"] == float(np.mean(r["ssim"]))
    # training views, a subset
    rt = t.evaluate([2, 0], split="train")
    sep = _separate_measurement(dev, t, [trc[2], trc[0]], [tri[2], tri[0]])
    assert rt["views"] == [2, 0] and [x for x, _ in sep] == rt["sse"] and [x for _, x in sep] == rt["ssim"]
    with pytest.raises(IndexError):
        t.evaluate([len(tec)])
    t.destroy()


@pytest.mark.parametrize("pipeline_depth,views_per_rank", [(1, 1), (2, 1), (1, 8), (2, 8)])
def test_evaluate_leaves_the_training_trajectory_alone(hip_device, pipeline_depth, views_per_rank):
    """13 steps across two densify events, evaluate every 3 steps vs never: cloud, SH rows and optimizer state equal bit for bit."""
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 8)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images, every=4)
    out = []
    for evaluating in (False, True):
        t = _trainer(dev, cfg, g, sh, trc, tri, pipeline_depth=pipeline_depth, views_per_rank=views_per_rank)
        t.setEvaluationViews(tec, tei)
        for i in range(13):
            t.step()
            if evaluating and i % 3 == 1:
                t.evaluate()
                t.evaluate([0], split="train")
        t.drain()
        st = t.optimizer.getStateBuffers()
        out.append(dict(n=t.getPointCount(), it=t.getIteration(), g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32),
                        **{k: st[k].read(np.uint32) for k in st}))
        t.destroy()
    assert out[0]["n"] == out[1]["n"] != 5000, "the run crosses densify rebuilds"
    assert out[0]["it"] == out[1]["it"] == 13
    for k in out[0]:
        if k not in ("n", "it"):
            assert_bits_equal(out[1][k], out[0][k], f"evaluating vs not: {k}")


def test_evaluate_other_sizes_and_overflow(hip_device):
    """Eval views of another size than the training views, with evaluate's lists far too small at first: the result equals a run whose lists
    are large, and the overflow is never reported from the truncated render."""
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 6)
    _, _, ecams, eimgs = _views(dev, cfg, 3, width=96, height=200, radius=0.8)
    _, _, ecams2, eimgs2 = _views(dev, cfg, 2, width=200, height=72, radius=0.6)
    ecams, eimgs = ecams + ecams2, eimgs + eimgs2
    res = []
    for small in (False, True):
        t = _trainer(dev, cfg, g, sh, cameras, images, densify=False)
        t.setEvaluationViews(ecams, eimgs)
        for _ in range(5):
            t.step()
        if small:
            t.evalMaxTileEntries = 256
            with pytest.warns(RuntimeWarning, match="evaluation tile-entry lists grown"):
                r = t.evaluate()
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                r = t.evaluate()
        sep = _separate_measurement(dev, t, ecams, eimgs)
        assert r["sse"] == [x for x, _ in sep] and r["ssim"] == [x for _, x in sep]
        res.append(r)
        t.destroy()
    assert res[0]["sse"] == res[1]["sse"] and res[0]["ssim"] == res[1]["ssim"]
    assert all(0.0 < s < 1.0 for s in res[0]["ssim"])


def test_held_out_psnr_and_ssim_rise_over_training(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=4000, width=160, height=128, sh_deg=0, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 24)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images)
    assert len(tec) == 3 and len(trc) == 21
    # the model: the target's geometry with every Gaussian's colour scrambled (a structural error, which SSIM sees -- the synthetic cloud's own
    # error against the target is a brightness shift, to which SSIM is nearly blind)
    tg, tsh = synth.make_target_scene(g, sh)
    h16 = tsh.copy().view(np.uint16).reshape(-1, 48)
    dc = h16[:, 0:3].view(np.float16).astype(np.float32) + np.random.default_rng(7).normal(0.0, 0.5, (len(h16), 3)).astype(np.float32)
    h16[:, 0:3] = synth.f32_to_f16_bits(dc)
    t = _trainer(dev, cfg, tg, h16.view(np.uint32).reshape(-1, 24), trc, tri, seed=11, densify=False)
    # colours and opacities learn, the geometry stays (the first steps of the reference's uncorrected Adam move it far: DESIGN.md)
    t.setOptimizerHyperparameters(dict(lr_pos=0.0, lr_rot=0.0, lr_scale=0.0))
    t.setEvaluationViews(tec, tei)
    r0 = t.evaluate()
    for _ in range(200):
        t.step()
    r1 = t.evaluate()
    print(f"held-out: PSNR {r0['mean_psnr']:.3f} -> {r1['mean_psnr']:.3f} dB, SSIM {r0['mean_ssim']:.5f} -> {r1['mean_ssim']:.5f}")
    assert r1["mean_psnr"] > r0["mean_psnr"] + 0.5
    assert r1["mean_ssim"] > r0["mean_ssim"]
    t.destroy()
