"""GPU: per-Gaussian render contribution (csrc/contrib.hip) and contribution-based pruning.  The records against the float64
restatement (tests/contrib64.py) fed with the GPU's own forward stages and against the depth kernel's weight-sum image, determinism, accumulation over
views and replays, the non-finite scenes, that pruning what was never composited changes no pixel, the Trainer surface, and the state errors."""
import random
import warnings

import numpy as np
import pytest

from webdgs_amd import _lib, ops, synth

import harness
from harness import assert_bits_equal
from test_contrib_reference import SCENES, contrib64_of
from test_depth_reference import scene_config
from test_gpu_eval import _trainer, _views
from test_gpu_nan import CHUNK_EDGE_PILES, NAN16, chunk_edge_scene, long_list_scene, poisoned, tile_list_lengths

pytestmark = pytest.mark.gpu

EPS = 2e-6   # per active pair: 2^-24 truncation + 1e-6 for the f32 A (test_depth_reference's bound) + 16 * 2^-24 for the alpha's roundings


def _records(pipe, into=None):
    """forward + encodeContribution into a (new, zeroed) buffer: the buffer."""
    buf = into if into is not None else ops.createContributionBuffer(pipe.dev, pipe.cfg.num_points)
    pipe.forward()
    pipe.rast.encodeContribution(None, buf)
    pipe.dev.synchronize()
    return buf


def _raw(buf, n):
    return buf.read(np.uint8, 16 * n).view(ops.CONTRIBUTION_DTYPE)


def _assert_records_match_float64(pipe, buf, name, exact_pixels):
    cfg = pipe.cfg
    got = ops.readContribution(buf, cfg.num_points)
    c = contrib64_of(pipe.collect_forward(), cfg)
    b_sum = c["pixels"] * EPS + c["slack_sum"]
    e_sum = np.abs(got["weight_sum"] - c["weight_sum"])
    b_max = EPS + c["slack_max"]
    e_max = np.abs(got["max_weight"].astype(np.float64) - c["max_weight"])
    e_pix = np.abs(got["pixels"].astype(np.int64) - c["pixels"])
    seen = c["pixels"] > 0
    r_sum = (e_sum[seen] / b_sum[seen]).max() if seen.any() else 0.0
    print(f"contribution accuracy {name}: worst |weight_sum - ws64| / (pixels eps + slack) = {r_sum:.3f}, worst |max_weight - max64| / (eps + slack) = "
          f"{(e_max / b_max).max():.3f}, pixel counts differing on {int((e_pix > 0).sum())} Gaussians (slack allows {int((c['slack_pixels'] > 0).sum())}), "
          f"Gaussians with weight {int(seen.sum())} of {cfg.num_points}, surely_zero {int(c['surely_zero'].sum())}, slack {c['slack_sum'].sum():.4g}")
    assert np.all(e_sum <= b_sum), f"{name}: weight sum off by {r_sum:.2f} x the bound"
    assert np.all(e_max <= b_max), f"{name}: max weight off by {(e_max / b_max).max():.2f} x the bound"
    assert np.all(e_pix <= c["slack_pixels"]), f"{name}: pixel counts differ beyond the slack on {int((e_pix > c['slack_pixels']).sum())} Gaussians"
    if exact_pixels:
        assert c["slack_pixels"].sum() == 0 and np.array_equal(got["pixels"].astype(np.int64), c["pixels"])
    z = c["surely_zero"]
    assert not got["sum_q"][z].any() and not got["max_weight"][z].any() and not got["pixels"][z].any(), f"{name}: weight on a Gaussian behind saturated pixels"
    assert got["max_weight"].max() <= np.float32(0.99)
    assert np.array_equal(got["weight_sum"], got["sum_q"].astype(np.float64) * 2.0 ** -24)


@pytest.mark.parametrize("name", SCENES)
def test_records_match_float64(hip_device, name):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        buf = _records(pipe)
        _assert_records_match_float64(pipe, buf, name, exact_pixels=name in ("sparse", "c1"))
        buf.destroy()
    finally:
        pipe.destroy()


def _list_lengths(fw, cfg):
    """L(p) summed over the image's pixels: each tile's list length times its pixels inside the image."""
    tiles = (fw["sorted_keys"] >> np.uint32(16)).astype(np.int64) - 1
    ntx, nty = (cfg.width + 15) // 16, (cfg.height + 15) // 16
    per_tile = np.bincount(tiles[(tiles >= 0) & (tiles < ntx * nty)], minlength=ntx * nty).reshape(nty, ntx)
    wpix = np.minimum(16, cfg.width - 16 * np.arange(ntx))
    hpix = np.minimum(16, cfg.height - 16 * np.arange(nty))
    return int((per_tile * np.outer(hpix, wpix)).sum())


def _identity_scenes():
    for name in SCENES:
        cfg = scene_config(name)
        yield (name, cfg) + harness.scene(cfg)
    cfg, g, sh, cam, _ = long_list_scene("sparse")
    yield "long lists (10 400 entries in one tile)", cfg, g, sh, cam


def _assert_weights_sum_to_the_weight_image(pipe, buf, what, least_entries):
    """buf: the records of pipe's last frame."""
    cfg = pipe.cfg
    pipe.rast.encodeDepth(None, ("weight_sum",))
    pipe.dev.synchronize()
    image = pipe.rast.getDepthTextureView("weight_sum").read(np.float32).astype(np.float64)
    got = ops.readContribution(buf, cfg.num_points)
    fw = pipe.collect_forward()
    assert int(fw["stats"][0]) >= least_entries
    bound = _list_lengths(fw, cfg) * 1.5 * 2.0 ** -24
    diff = abs(float(got["sum_q"].sum()) * 2.0 ** -24 - image.sum())
    print(f"contribution vs depth {what}: |sum_g - sum_p| = {diff:.3e}, bound {bound:.3e} ({diff / bound:.3f})")
    assert np.isfinite(image).all() and diff <= bound, f"{what}: {diff} > {bound}"


def test_weights_sum_to_the_depth_kernels_weight_image(hip_device):
    """GPU only, no float64: every active pair's w is added to one pixel's weight sum by depth.hip and, truncated to 2^-24, to one Gaussian's sum_q here."""
    for what, cfg, g, sh, cam in _identity_scenes():
        pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
        try:
            buf = _records(pipe)
            _assert_weights_sum_to_the_weight_image(pipe, buf, what, 10_400 if what.startswith("long") else 1)
            buf.destroy()
        finally:
            pipe.destroy()


def test_lists_that_end_at_the_chunk_edges(hip_device):
    """Tile lists of 1, 63, 64, 65, 128 and 129 entries (test_gpu_nan.chunk_edge_scene), none of which saturates a pixel: the walk's chunks of 64 end with
    the list, one entry before it and one entry after it.  The records against float64, pixel counts exactly, and against the depth kernel's weight image."""
    cfg, g, sh, cam = chunk_edge_scene()
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        buf = _records(pipe)
        lens = tile_list_lengths(pipe.collect_forward()["tile_ranges"])
        ntx = (cfg.width + 15) // 16
        assert {t: int(lens[t[1] * ntx + t[0]]) for t in CHUNK_EDGE_PILES} == CHUNK_EDGE_PILES, "the scene is not the one this test is about"
        _assert_records_match_float64(pipe, buf, "chunk edges", exact_pixels=True)
        _assert_weights_sum_to_the_weight_image(pipe, buf, "chunk edges", 581)
        buf.destroy()
    finally:
        pipe.destroy()


def test_determinism_accumulation_and_replay(hip_device):
    dev = hip_device
    cfg = scene_config("c2-20k")
    g, sh, _ = harness.scene(cfg)
    cams = synth.circle_cameras(cfg, 3)
    n = cfg.num_points
    pipe = harness.HipPipeline(dev, cfg, g, sh, cams[0])
    try:
        single = []
        for cam in cams:
            pipe.camera.write(cam)
            a, b = _records(pipe), _records(pipe)
            single.append(_raw(a, n).copy())
            assert_bits_equal(_raw(b, n), single[-1], "two runs of one view")
            a.destroy(); b.destroy()
        assert single[0]["pixels"].sum() > 0 and not np.array_equal(single[0], single[1])
        want = np.zeros(n, ops.CONTRIBUTION_DTYPE)
        want["sum_q"] = sum(s["sum_q"] for s in single)
        want["pixels"] = sum(s["pixels"] for s in single)
        want["max_bits"] = np.maximum.reduce([s["max_bits"] for s in single])
        for order in ((0, 1, 2), (2, 0, 1)):
            acc = ops.createContributionBuffer(dev, n)
            for v in order:
                pipe.camera.write(cams[v])
                _records(pipe, into=acc)
            assert_bits_equal(_raw(acc, n), want, f"views {order} into one buffer")
            acc.destroy()
        # a recorded command buffer adds once per submission
        pipe.camera.write(cams[0])
        acc = ops.createContributionBuffer(dev, n)
        with dev.createCommandEncoder("contribution", record=True) as enc:
            pipe.fwd.encode(enc)
            pipe.rast.encode(enc, cfg.width, cfg.height)
            pipe.rast.encodeContribution(enc, acc)
            cmd = enc.finish()
        acc.clear()
        dev.queue.submit([cmd])
        dev.synchronize()
        assert_bits_equal(_raw(acc, n), single[0], "recording submitted once")
        dev.queue.submit([cmd])
        dev.synchronize()
        twice = _raw(acc, n)
        cmd.destroy()
        assert np.array_equal(twice["sum_q"], 2 * single[0]["sum_q"]) and np.array_equal(twice["pixels"], 2 * single[0]["pixels"])
        assert np.array_equal(twice["max_bits"], single[0]["max_bits"])
        acc.destroy()
    finally:
        pipe.destroy()


def _non_finite_scenes():
    cfg, g, sh, cam, _ = long_list_scene("pile-up")
    yield "long lists pile-up", cfg, g, sh, cam
    cfg4 = harness.small_config("c1", num_points=4000, width=64, height=48)
    g, sh, cam = poisoned(cfg4, "position", NAN16, every=2)
    yield "pile behind a dead block", cfg4, g, sh, cam
    g, sh, cam = poisoned(cfg4, "opacity", NAN16, every=2)
    yield "NaN opacities", cfg4, g, sh, cam


def test_non_finite_scenes(hip_device):
    for what, cfg, g, sh, cam in _non_finite_scenes():
        pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
        try:
            a, b = _records(pipe), _records(pipe)
            got = ops.readContribution(a, cfg.num_points)
            assert np.isfinite(got["max_weight"]).all() and got["max_weight"].max() <= np.float32(0.99) and got["max_weight"].min() >= 0, what
            assert got["pixels"].sum() > 0, what
            assert np.all((got["pixels"] == 0) <= (got["sum_q"] == 0)), what
            assert_bits_equal(_raw(b, cfg.num_points), _raw(a, cfg.num_points), f"{what}: two runs")
            a.destroy(); b.destroy()
        finally:
            pipe.destroy()


def _frames(pipe, cams):
    out = []
    for cam in cams:
        pipe.camera.write(cam)
        pipe.forward()
        out.append((pipe.rast.getOutputTextureView().read(np.uint32).copy(), pipe.rast.getAlphaTextureView().read(np.uint32).copy()))
    return out


def prune_never_composited(dev, cfg, g, sh, cams):
    """The ops-level sequence: statistics over the views, decision min_pixels = 1, prefix sum, total, scatter.  (records, new cloud, frames before)."""
    n = cfg.num_points
    pipe = harness.HipPipeline(dev, cfg, g, sh, cams[0])
    dp = ops.DensifyPrunePass(dev)
    try:
        before = _frames(pipe, cams)
        stats = ops.createContributionBuffer(dev, n)
        for cam in cams:
            pipe.camera.write(cam)
            _records(pipe, into=stats)
        rec = _raw(stats, n).copy()
        dp.ensureSize(n)
        dec = dp.encodeContributionDecision(None, n, stats, dict(minPixels=1))
        offsets = dp.encodePrefixSum(None)
        dp.encodeTotalOut(None)
        total = dp.readTotal()
        actions, counts = dec["actionBuffer"].read(np.uint32)[:n], dec["outCountBuffer"].read(np.uint32)[:n]
        out_pc = ops.allocatePointCloudLike(dev, pipe.pc, dict(numPoints=total))
        dp.encodeScatter(None, dict(pointCloud=pipe.pc, outOffsetBuffer=offsets, outNumPoints=total, resetNewOptimizerState=False), dict(outPointCloud=out_pc))
        dev.synchronize()
        new_g = out_pc.gaussian_3d_buffer.read(np.uint32)[:6 * total].reshape(total, 6).copy()
        new_sh = out_pc.sh_buffer.read(np.uint32)[:24 * total].reshape(total, 24).copy()
        out_pc.gaussian_3d_buffer.destroy(); out_pc.sh_buffer.destroy(); stats.destroy()
        return rec, actions, counts, total, new_g, new_sh, before
    finally:
        dp.destroy()
        pipe.destroy()


def test_pruning_what_was_never_composited_changes_no_pixel(hip_device):
    dev = hip_device
    cfg = scene_config("big-splats")
    g, sh, _ = harness.scene(cfg)
    cams = synth.circle_cameras(cfg, 3)
    rec, actions, counts, total, new_g, new_sh, before = prune_never_composited(dev, cfg, g, sh, cams)
    keep = rec["pixels"] >= 1
    assert total == int(keep.sum()) and 0 < total < cfg.num_points // 2, (total, cfg.num_points)
    assert np.array_equal(counts, keep.astype(np.uint32)) and np.array_equal(actions, np.where(keep, 0, 3).astype(np.uint32))
    assert_bits_equal(new_g, np.asarray(g, np.uint32).reshape(-1, 6)[keep], "kept Gaussian rows")
    assert_bits_equal(new_sh, np.asarray(sh, np.uint32).reshape(-1, 24)[keep], "kept SH rows")
    vcfg = synth.SceneConfig(cfg.config_id, total, cfg.width, cfg.height, cfg.sh_deg, cfg.fy, cfg.s0, cfg.name)
    pruned = harness.HipPipeline(dev, vcfg, new_g, new_sh, cams[0])
    try:
        after = _frames(pruned, cams)
    finally:
        pruned.destroy()
    for v, ((rgba0, alpha0), (rgba1, alpha1)) in enumerate(zip(before, after)):
        assert_bits_equal(rgba1, rgba0, f"view {v}: rgba8 after pruning")
        assert_bits_equal(alpha1, alpha0, f"view {v}: alpha texture after pruning")


STATE_ROWS = dict(optPosBuffer=12, optRotBuffer=12, optScaleBuffer=12, optOpacityBuffer=3, paramSH=48, stateSH=96)   # u32 words per Gaussian
TRAINER_CFG = dict(base="c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)   # test_gpu_eval's small setting


def _state(t):
    st = t.optimizer.getStateBuffers()
    n = t.getPointCount()
    return {k: st[k].read(np.uint32)[:w * n].reshape(n, w).copy() for k, w in STATE_ROWS.items()}


def test_trainer_prune_by_contribution(hip_device):
    dev = hip_device
    cfg = harness.small_config(**TRAINER_CFG)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    try:
        for _ in range(20):
            t.step()
        sse = t.evaluate(split="train")["sse"]
        stats = t.contributionStats()
        assert stats["views"] == [0, 1, 2, 3] and len(stats["pixels"]) == cfg.num_points and stats["sum_q"].dtype == np.uint64
        assert np.array_equal(stats["weight_sum"], stats["sum_q"].astype(np.float64) * 2.0 ** -24) and stats["max_weight"].dtype == np.float32
        one = t.contributionStats([2])
        assert one["views"] == [2] and np.all(one["pixels"] <= stats["pixels"]) and one["pixels"].sum() < stats["pixels"].sum()
        keep = stats["pixels"] >= 1
        t.flushPointCloud()
        rows_g = t.pointCloud.gaussian_3d_buffer.read(np.uint32)[:6 * cfg.num_points].reshape(-1, 6).copy()
        state, it, opt_it, rng = _state(t), t.getIteration(), t.optimizer.getIteration(), t._rng.getstate()
        r = t.pruneByContribution(minPixels=1)
        assert r == dict(before=cfg.num_points, after=int(keep.sum()), pruned=int((~keep).sum())) and r["pruned"] > 0
        assert t.getPointCount() == int(keep.sum())
        assert_bits_equal(t.pointCloud.gaussian_3d_buffer.read(np.uint32)[:6 * r["after"]].reshape(-1, 6), rows_g[keep], "survivors' Gaussian rows")
        after = _state(t)
        for k in STATE_ROWS:
            assert_bits_equal(after[k], state[k][keep], f"survivors' optimizer array {k}")
        assert t.getIteration() == it == 20 and t.optimizer.getIteration() == opt_it and t._rng.getstate() == rng
        assert t.evaluate(split="train")["sse"] == sse, "pruning what no training view composited changed a training view"
        t.step()
        t.drain()
        assert t.getIteration() == 21
        # a fraction: the Gaussians numpy selects from the read-back
        n = t.getPointCount()
        s = t.contributionStats()["sum_q"]
        k = int(np.floor(0.3 * n))
        thr = np.sort(s)[k - 1]
        gone = s < thr
        rows_g = t.pointCloud.gaussian_3d_buffer.read(np.uint32)[:6 * n].reshape(-1, 6).copy()
        r = t.pruneByContribution(fraction=0.3)
        assert r["pruned"] == int(gone.sum()) <= k and r["after"] == n - r["pruned"] == t.getPointCount() and r["pruned"] > 0
        assert_bits_equal(t.pointCloud.gaussian_3d_buffer.read(np.uint32)[:6 * r["after"]].reshape(-1, 6), rows_g[~gone], "fraction: the survivors")
        # nothing to prune, everything to prune, no criterion
        assert t.pruneByContribution(fraction=1e-9)["pruned"] == 0
        n = t.getPointCount()
        with pytest.warns(RuntimeWarning, match="every Gaussian"):
            assert t.pruneByContribution(minMaxWeight=0.995) == dict(before=n, after=n, pruned=0)
        with pytest.raises(ValueError):
            t.pruneByContribution()
        with pytest.raises(IndexError):
            t.contributionStats([4])
        t.step()
    finally:
        t.destroy()


def test_prune_by_contribution_needs_one_rank(hip_device):
    from webdgs_amd.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.world_size = 2
    with pytest.raises(RuntimeError, match="world_size"):
        t.pruneByContribution(minPixels=1)


def _trajectory(dev, cfg, g, sh, cameras, imgs, depth, watching):
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False, pipeline_depth=depth)
    try:
        for i in range(20):
            t.step()
            if watching and i % 4 == 1:
                s = t.contributionStats([i % 4, 0] if i % 8 == 1 else None)
                assert s["pixels"].sum() > 0
        t.drain()
        return dict(_state(t), g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32), rng=np.array(t._rng.getstate()[1]))
    finally:
        t.destroy()


@pytest.mark.parametrize("depth", [1, 2])
def test_trainer_trajectory_is_untouched_by_contribution_stats(hip_device, depth):
    cfg = harness.small_config(**TRAINER_CFG)
    g, sh, cameras, imgs = _views(hip_device, cfg, 4)
    plain = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, False)
    watched = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, True)
    for k in plain:
        assert_bits_equal(watched[k], plain[k], f"20 steps with contributionStats between them, pipeline depth {depth}: {k}")


def test_state_errors(hip_device):
    dev = hip_device
    cfg = scene_config("sparse")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    buf = ops.createContributionBuffer(dev, cfg.num_points + 1)
    dp = ops.DensifyPrunePass(dev)
    try:
        assert not buf.read(np.uint8).any() and buf.size == 16 * (cfg.num_points + 1)
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeContribution(None, buf)            # nothing encoded at all
        pipe.fwd.encode(None)
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeContribution(None, buf)            # the forward pass alone
        pipe.forward()
        with pytest.raises(_lib.WdgsError) as e:
            pipe.rast.encodeContribution(None, dev.view(buf.ptr + 8, buf.size - 8))
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(ValueError):
            pipe.rast.encodeContribution(None, dev.view(buf.ptr, 16))   # too small for the cloud
        pipe.fwd.setRenderMode("pointcloud")
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeContribution(None, buf)
        assert not buf.read(np.uint8).any(), "a refused call wrote"
        pipe.fwd.setRenderMode("gaussian")
        pipe.forward()
        pipe.rast.encodeContribution(None, buf)
        dev.synchronize()
        assert ops.readContribution(buf, cfg.num_points)["pixels"].sum() > 0
        assert not buf.read(np.uint8, 16, offset=16 * cfg.num_points).any(), "a record past the cloud was written"
        for rule in ({}, dict(minPixels=0, minMaxWeight=0.0)):
            with pytest.raises(_lib.WdgsError) as e:
                dp.encodeContributionDecision(None, cfg.num_points, buf, rule)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.WdgsError) as e:
            dp.encodeContributionDecision(None, cfg.num_points, dev.view(buf.ptr + 8, buf.size - 8), dict(minPixels=1))
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(ValueError):
            dp.encodeContributionDecision(None, cfg.num_points, buf, dict(minPixel=1))
    finally:
        dp.destroy()
        buf.destroy()
        pipe.destroy()
