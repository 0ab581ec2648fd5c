"""GPU: the re-allocation paths of the op structs (csrc/api.hip, devmem.h) -- per-tile tables and images that follow the viewport, per-Gaussian
buffers that follow the cloud, depth images across a size change, optimizer state handed from one optimizer to the next.  Each buffer grows, is
reused while larger than needed and grows again; after every change the passes must produce the oracle's bits (or a freshly built pass's)."""
import ctypes as C

import numpy as np
import pytest

from webdgs_amd import _lib, ops, synth
from webdgs_amd._lib import check

import harness
from harness import assert_bits_equal

pytestmark = pytest.mark.gpu


def _cfg(n, w, h, **kw):
    return harness.small_config("c1", num_points=n, width=w, height=h, fy=0.9 * max(w, h), **kw)


def _target(w, h):
    return np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _set_viewport(pipe, cfg):
    """The pipeline's passes and its camera follow ``cfg``'s viewport; returns the camera block."""
    cam = synth.identity_camera(cfg)
    pipe.camera.write(cam)
    pipe.fwd.setViewport(cfg.width, cfg.height)
    pipe.bwd.setViewport(cfg.width, cfg.height)
    pipe.cfg = cfg
    return cam


def _oracle_args(cfg):
    return synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)


def test_viewport_walk_there_and_back(hip_device, orc):
    """One pipeline through 16x16 (one tile) -> 272x48 -> 16x16 -> 48x272: range table, non-finite stamps, long-list marks, the rasterizer's images and
    the loss / metric images grow, are reused while larger than needed, and change shape again.  At every size the forward pass, the composite and
    the loss image equal the oracle's."""
    dev, n = hip_device, 3000
    g, sh, cam = harness.scene(_cfg(n, 16, 16))
    pipe = harness.HipPipeline(dev, _cfg(n, 16, 16), g, sh, cam)
    try:
        for w, h in ((16, 16), (272, 48), (16, 16), (48, 272)):
            cfg = _cfg(n, w, h)
            cam = _set_viewport(pipe, cfg)
            target = _target(w, h)
            tbuf = dev.bufferFrom(target)
            pipe.forward()
            pipe.bwd.encode(None, pipe.rast.getOutputTextureView(), tbuf, pipe.backward_resources())
            dev.synchronize()
            got = pipe.collect_forward()
            ref = orc.forward(g, sh, cam, *_oracle_args(cfg))
            what = f"{w}x{h}"
            assert got["total_entries"] == ref["total_entries"] > 0, what
            for k in ("rgba8", "n_contrib", "final_T", "tile_ranges"):
                assert_bits_equal(got[k], ref[k], f"{what}: {k}")
            loss = pipe.bwd.getLossTextureView().read(np.float32).reshape(h, w, 4)
            assert_bits_equal(loss, orc.loss_grad(ref["rgba8"], target, orc.training_config()), f"{what}: loss image")
    finally:
        pipe.destroy()


def _tile_sorted_cloud(orc, g, sh, cfg):
    """The Gaussians of (g, sh) that touch exactly one tile of ``cfg``'s grid, in the order of their tiles: their entries leave emit sorted by tile, so
    the range search over UNSORTED entries (encode(skipSort)) is well defined."""
    fw = orc.forward(g, sh, synth.identity_camera(cfg), *_oracle_args(cfg))
    idx = np.flatnonzero(fw["tile_counts"] == 1)
    tile = fw["keys"][fw["tile_offsets"][idx]] >> 16
    order = idx[np.argsort(tile, kind="stable")]
    return np.ascontiguousarray(g[order]), np.ascontiguousarray(sh[order])


def test_the_rasterizers_own_range_table_follows_the_viewport(hip_device, orc):
    """The rasterizer builds a range table of its own when the forward pass built none: under compat_caps (the reference's plain sort) and after
    encode(skipSort).  Both from 16x16 to 208x112: the table is re-allocated, and table, image and n_contrib equal the oracle's."""
    dev = hip_device
    big = _cfg(2000, 208, 112)
    g, sh, _ = harness.scene(big)

    # compat_caps: sorted entries, at most 32 batches of 256 per tile
    pipe = harness.HipPipeline(dev, _cfg(2000, 16, 16), g, sh, synth.identity_camera(_cfg(2000, 16, 16)), compat_caps=True)
    try:
        for w, h in ((16, 16), (208, 112)):
            cfg = _cfg(2000, w, h)
            cam = _set_viewport(pipe, cfg)
            pipe.forward()
            got = pipe.collect_forward()
            ref = orc.forward(g, sh, cam, *_oracle_args(cfg), max_batches=32)
            assert int(got["stats"][2]) == 0 and got["total_entries"] == ref["total_entries"] > 0
            for k in ("tile_ranges", "rgba8", "n_contrib"):
                assert_bits_equal(got[k], ref[k], f"compat_caps {w}x{h}: {k}")
    finally:
        pipe.destroy()

    # encode(skipSort): entries in emission order, which for this cloud is tile order
    g2, sh2 = _tile_sorted_cloud(orc, g, sh, big)
    n2 = g2.shape[0]
    assert n2 > 300
    pipe = harness.HipPipeline(dev, _cfg(n2, 16, 16), g2, sh2, synth.identity_camera(_cfg(n2, 16, 16)))
    try:
        for w, h in ((16, 16), (208, 112)):
            cfg = _cfg(n2, w, h)
            cam = _set_viewport(pipe, cfg)
            pipe.fwd.encode(None, dict(skipSort=True))
            pipe.rast.encode(None, w, h)
            dev.synchronize()
            got = pipe.collect_forward()
            st, ti = _oracle_args(cfg)
            ref = orc.forward(g2, sh2, cam, st, ti)
            e = ref["total_entries"]
            keys, vals = ref["keys"][:e], ref["values"][:e]
            assert e > 0 and (np.diff((keys >> 16).astype(np.int64)) >= 0).all(), "the emission order of this cloud is tile order"
            ranges = orc.tile_ranges(keys, e, int(ti[2]))
            rgba, _, ncontrib = orc.rasterize(st, ti, ref["splats"], ranges, keys, vals, e)
            assert_bits_equal(got["sorted_keys"], keys, f"skipSort {w}x{h}: entries in emission order")
            assert_bits_equal(got["tile_ranges"], ranges, f"skipSort {w}x{h}: tile_ranges")
            assert_bits_equal(got["rgba8"], rgba, f"skipSort {w}x{h}: rgba8")
            assert_bits_equal(got["n_contrib"], ncontrib, f"skipSort {w}x{h}: n_contrib")
    finally:
        pipe.destroy()


def test_point_count_walk(hip_device, orc):
    """setPointCloud on both passes through 300 -> 5 000 (past the 25 % headroom: re-allocated) -> 200 (far below) -> 260 (inside the old block), a
    full step after each: every forward stage, the accumulators and the packed gradients equal the oracle's."""
    dev = hip_device
    w, h = 96, 80
    g, sh, cam = harness.scene(_cfg(5000, w, h))
    st, ti = _oracle_args(_cfg(5000, w, h))
    target = _target(w, h)
    tbuf = dev.bufferFrom(target)
    pipe = harness.HipPipeline(dev, _cfg(300, w, h), g[:300], sh[:300], cam)
    try:
        for n in (300, 5000, 200, 260):
            gn, shn = np.ascontiguousarray(g[:n]), np.ascontiguousarray(sh[:n])
            pc = ops.createPointCloud(dev, gn, shn, pipe.cfg.sh_deg)
            assert pipe.fwd.setPointCloud(pc) and pipe.bwd.setPointCloud(pc)
            pipe.pc, pipe.cfg = pc, _cfg(n, w, h)
            if pipe.opt is not None:
                pipe.opt.destroy()
                pipe.opt = None
            pipe.train_step(tbuf)
            dev.synchronize()
            got = pipe.collect_forward()
            ref = orc.view_gradients(gn, shn, cam, st, ti, target)
            vis = ref["tile_counts"] > 0
            assert vis.sum() > 0 and got["total_entries"] == ref["total_entries"] and int(got["stats"][1]) == int(vis.sum()), n
            for k in ("tile_counts", "tile_offsets", "tile_ranges", "n_contrib", "final_T", "rgba8"):
                assert_bits_equal(got[k], ref[k], f"{n} Gaussians: {k}")
            for k in ("splats", "depths"):
                assert_bits_equal(got[k][vis], ref[k][vis], f"{n} Gaussians: {k} of the visible ones")
            for k in ("sorted_keys", "sorted_values"):
                assert_bits_equal(got[k], ref[k][:ref["total_entries"]], f"{n} Gaussians: {k}")
            acc = harness.acc_to_reference_layout(pipe.bwd.getAccumulatorsBuffer().read(np.int32), n)
            for a, k in zip(acc, ("grad_means", "grad_conics", "grad_opacity", "grad_colors")):
                assert_bits_equal(a, ref[k], f"{n} Gaussians: accumulators {k}")
            assert_bits_equal(pipe.bwd.getGradientsBuffer().read(np.uint32).reshape(-1, 8)[:n], ref["gradients"], f"{n} Gaussians: packed gradients")
    finally:
        pipe.destroy()


def test_depth_images_across_a_size_change(hip_device):
    """encodeDepth with every kind at 64x48, then a viewport of 208x112: the images are re-made per kind as kinds are asked for, each equal to the same
    call on a pipeline built at 208x112, and a kind not asked for since the change is reported as not encoded."""
    dev = hip_device
    small, big = _cfg(4000, 64, 48), _cfg(4000, 208, 112)
    g, sh, _ = harness.scene(big)
    pipe = harness.HipPipeline(dev, small, g, sh, synth.identity_camera(small))
    fresh = harness.HipPipeline(dev, big, g, sh, synth.identity_camera(big))
    try:
        pipe.forward()
        pipe.rast.encodeDepth(None, ("expected", "median", "weight_sum"))
        dev.synchronize()
        assert pipe.rast.getDepthTextureView("median").read(np.float32).size == 64 * 48
        _set_viewport(pipe, big)
        for p in (pipe, fresh):
            p.forward()
        for asked, missing in (("median", "expected"), ("expected", "weight_sum")):
            for p in (pipe, fresh):
                p.rast.encodeDepth(None, (asked,))
            dev.synchronize()
            a, b = (p.rast.getDepthTextureView(asked).read(np.float32) for p in (pipe, fresh))
            assert a.size == 208 * 112 and np.isfinite(a).any() and a.any()
            assert_bits_equal(a, b, f"{asked} depth after the size change")
            with pytest.raises(_lib.StateError, match="not encoded yet"):
                pipe.rast.getDepthTextureView(missing)
    finally:
        pipe.destroy()
        fresh.destroy()


_STATE_ARRAYS = [f for f, _ in _lib.OptimizerState._fields_]


def _optimizer(dev, pc, initial=None, iteration=0):
    """wdgs_optimizer_create with library-owned state: allocated by the library, or ``initial`` (arrays from wdgs_optimizer_release_state) adopted with ownership."""
    h = C.c_void_p()
    check(dev.lib.wdgs_optimizer_create(dev.handle, pc.num_points, None, pc.gaussian_3d_buffer.ptr, pc.sh_buffer.ptr,
                                        C.byref(initial) if initial is not None else None, 1 if initial is not None else 0, iteration, C.byref(h)))
    return h


def _step(pipe, opt, tbuf):
    pipe.fwd.encode(None)
    pipe.rast.encode(None, pipe.cfg.width, pipe.cfg.height)
    pipe.bwd.encode(None, pipe.rast.getOutputTextureView(), tbuf, pipe.backward_resources())
    check(pipe.dev.lib.wdgs_optimizer_step(opt, pipe.pc.gaussian_3d_buffer.ptr, pipe.pc.sh_buffer.ptr, pipe.bwd.getGradientsBuffer().ptr,
                                           pipe.fwd.getResources()["tileCountsBuffer"].ptr))


def _read_state(dev, opt, n):
    st, sizes = _lib.OptimizerState(), (C.c_size_t * 6)()
    check(dev.lib.wdgs_optimizer_get_state(opt, C.byref(st)))
    check(dev.lib.wdgs_optimizer_state_sizes(n, C.byref(sizes)))
    return {f: dev.view(getattr(st, f), sizes[i]).read(np.uint32) for i, f in enumerate(_STATE_ARRAYS)}


def test_optimizer_state_hand_over(hip_device):
    """Two steps, the state released (wdgs_optimizer_release_state: the hand-over of a densify swap), the optimizer destroyed, a second optimizer built
    on the arrays WITH ownership, two more steps, destroyed: the six arrays equal those of one optimizer stepped four times, and every block is back
    with the library (free + cached memory is no less than before the sequence)."""
    dev, lib = hip_device, hip_device.lib
    cfg = _cfg(2000, 96, 80)
    g, sh, cam = harness.scene(cfg)
    tbuf = dev.bufferFrom(_target(cfg.width, cfg.height))
    one, two = (harness.HipPipeline(dev, cfg, g, sh, cam) for _ in range(2))
    try:
        # the reference: one optimizer, four steps (its blocks, back in the cache, are what the sequence below is served from)
        opt = _optimizer(dev, one.pc)
        for _ in range(4):
            _step(one, opt, tbuf)
        want = _read_state(dev, opt, cfg.num_points)
        assert int(lib.wdgs_optimizer_get_iteration(opt)) == 4
        check(lib.wdgs_optimizer_destroy(opt))
        two.forward()   # (the passes' own first-use allocations -- range table, rasterizer images -- are not part of the sequence that is measured)
        dev.synchronize()
        before = dev.memoryInfo()

        first = _optimizer(dev, two.pc)
        for _ in range(2):
            _step(two, first, tbuf)
        handed = _lib.OptimizerState()
        check(lib.wdgs_optimizer_release_state(first, C.byref(handed)))
        assert all(getattr(handed, f) for f in _STATE_ARRAYS)
        check(lib.wdgs_optimizer_destroy(first))
        second = _optimizer(dev, two.pc, initial=handed, iteration=2)
        for _ in range(2):
            _step(two, second, tbuf)
        got = _read_state(dev, second, cfg.num_points)
        assert int(lib.wdgs_optimizer_get_iteration(second)) == 4
        check(lib.wdgs_optimizer_destroy(second))
        dev.synchronize()
        after = dev.memoryInfo()

        for f in _STATE_ARRAYS:
            assert want[f].any()
            assert_bits_equal(got[f], want[f], f"state after the hand-over: {f}")
        assert_bits_equal(two.pc.gaussian_3d_buffer.read(np.uint32), one.pc.gaussian_3d_buffer.read(np.uint32), "Gaussians after the hand-over")
        print(f"memory before {before}, after {after}")
        assert after["free"] + after["cached"] >= before["free"] + before["cached"], (before, after)
    finally:
        one.destroy()
        two.destroy()
