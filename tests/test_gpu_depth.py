"""GPU: the depth images (csrc/depth.hip).  The weight sum against the rasterizer's alpha texture bit for bit, expected and median
depth against the float64 restatement (tests/depth64.py) fed with the GPU's own forward stages, determinism and recording, that depth changes nothing
else, state errors, the presentation kernel, and the Viewer / backprojectDepth surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, images, loaders, ops, synth
from webdgs_amd.viewer import Viewer

import depth64 as d64
import harness
from harness import assert_bits_equal
from test_depth_reference import MASK_CAP, SCENES, depth64_of, scene_config
from test_gpu_eval import _trainer, _views
from test_gpu_nan import CHUNK_EDGE_PILES, INF16, NAN16, chunk_edge_scene, long_list_scene, poisoned, tile_list_lengths

pytestmark = pytest.mark.gpu

ALL = ("expected", "median", "weight_sum")


def _read(pipe, kinds=ALL):
    cfg = pipe.cfg
    return {k: pipe.rast.getDepthTextureView(k).read(np.float32).reshape(cfg.height, cfg.width).copy() for k in kinds}


def _depth(pipe, kinds=ALL):
    pipe.forward()
    pipe.rast.encodeDepth(None, kinds)
    pipe.dev.synchronize()
    return _read(pipe, kinds)


def _assert_weight_sum_is_alpha(pipe, got, what):
    """1.0f - A against the alpha texture, every pixel; a pixel whose sums are NaN must be a NaN in both."""
    alpha = pipe.rast.getAlphaTextureView().read(np.float32).reshape(got["weight_sum"].shape)
    with np.errstate(invalid="ignore"):
        mine = np.float32(1) - got["weight_sum"]
    nan = np.isnan(alpha)
    assert np.array_equal(nan, np.isnan(mine)), f"{what}: NaN pixels differ"
    assert_bits_equal(np.where(nan, np.float32(0), mine), np.where(nan, np.float32(0), alpha), f"{what}: 1 - weight_sum vs the alpha texture")
    return int(nan.sum())


@pytest.mark.parametrize("compat", [False, True], ids=["uncapped", "compatCaps"])
@pytest.mark.parametrize("name", list(SCENES))
def test_depth_images_match_float64(hip_device, name, compat):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    _assert_depth_images_match_float64(hip_device, cfg, g, sh, cam, name, compat)


def _assert_depth_images_match_float64(hip_device, cfg, g, sh, cam, name, compat=False):
    """The three depth images of one scene under one camera against depth64 fed with the GPU's own forward stages.  Returns the walk's statistics."""
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam, compat_caps=compat)
    try:
        got = _depth(pipe)
        assert _assert_weight_sum_is_alpha(pipe, got, name) == 0
        fw = pipe.collect_forward()
        A, D, M, near_sat, near_half, stats = depth64_of(fw, cfg, max_entries=8192 if compat else 0, probe=got["median"])
        assert near_sat.mean() <= MASK_CAP and near_half.mean() <= MASK_CAP, (near_sat.mean(), near_half.mean())
        zmax = float(np.abs(d64.decode_depths(fw["depths"])[fw["sorted_values"]]).max())
        # expected depth: one rounding per FMA, a few ulp of the deterministic exp on the weights that matter, one division
        tol = (stats["n_active"] + 32) * 2.0 ** -23
        err = np.abs(got["expected"].astype(np.float64) - D) / zmax
        keep = ~near_sat
        ratio = (err / tol)[keep]
        print(f"depth accuracy {name} compat={compat}: max |D - D64| / max|z| = {err[keep].max():.3e} (max|z| = {zmax:.4g}), worst share of the bound "
              f"(n_p + 32) 2^-23 = {ratio.max():.3f}, max n_p = {int(stats['n_active'].max())}, near_sat {near_sat.mean():.4%}, near_half {near_half.mean():.4%}")
        assert np.all(err[keep] <= tol[keep]), f"{name}: expected depth off by {ratio.max():.2f} x the bound"
        assert np.all(got["expected"][stats["n_active"] == 0] == 0)
        # median: a copy of one Gaussian's stored z
        sure = ~(near_sat | near_half)
        assert_bits_equal(got["median"][sure], M.astype(np.float32)[sure], f"{name}: median depth")
        assert np.all(stats["probe_in_box"][(got["median"] != 0)]), f"{name}: a median that is no record's z"
        # weight sum against float64 (the bit-level check above is the sharp one)
        assert np.abs(got["weight_sum"].astype(np.float64) - A)[keep].max() <= 1e-6
        return stats
    finally:
        pipe.destroy()


def test_c3_weight_sum_and_determinism(hip_device):
    cfg = synth.CONFIGS["c3"]
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        got = _depth(pipe)
        assert _assert_weight_sum_is_alpha(pipe, got, "c3") == 0
        again = _depth(pipe)
        for k in ALL:
            assert_bits_equal(again[k], got[k], f"c3 second encode: {k}")
        z = d64.decode_depths(pipe.fwd.getResources()["depthsBuffer"].read(np.uint32)[:cfg.num_points])
        seen = got["weight_sum"] > 0
        assert seen.mean() > 0.99
        assert got["expected"][seen].min() >= z[z > 0].min() and got["expected"][seen].max() <= np.nanmax(z)
        assert np.all(np.isin(got["median"][got["median"] != 0], z))
        assert np.array_equal(got["median"] != 0, got["weight_sum"] >= 0.5)
    finally:
        pipe.destroy()


def _special_scenes():
    cfg = harness.small_config("c1", num_points=700, width=64, height=48)
    for field, value in (("position", NAN16), ("opacity", NAN16), ("scale", INF16), ("z", 0xFE00)):
        g, sh, cam = poisoned(cfg, field, value)
        yield f"non-finite {field}", cfg, g, sh, cam
    cfg4 = harness.small_config("c1", num_points=4000, width=64, height=48)
    g, sh, cam = poisoned(cfg4, "position", NAN16, every=2)
    yield "pile behind a dead block", cfg4, g, sh, cam
    for kind in ("sparse", "faint", "pile-up"):
        cfg, g, sh, cam, _ = long_list_scene(kind)
        yield f"long lists {kind}", cfg, g, sh, cam


@pytest.mark.parametrize("compat", [False, True], ids=["uncapped", "compatCaps"])
def test_weight_sum_on_long_lists_and_non_finite_scenes(hip_device, compat):
    """The bit-level identity where the rasterizer takes its other routes: tiles stamped non-finite (the EXACT forms) and tile lists past 4 096 entries
    (the rasterizer's long-list tasks; the depth kernel walks them the plain way).  Finite pixels bit for bit, NaN pixels NaN in both."""
    nan_pixels = 0
    for what, cfg, g, sh, cam in _special_scenes():
        pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam, compat_caps=compat)
        try:
            got = _depth(pipe)
            nan_pixels += _assert_weight_sum_is_alpha(pipe, got, what)
            nan = np.isnan(got["weight_sum"])
            assert np.all(got["expected"][nan] == 0), f"{what}: a pixel with NaN sums has expected depth 0"
            fin = ~nan
            assert np.array_equal((got["median"] != 0)[fin], (got["weight_sum"] >= 0.5)[fin]), what
            again = _depth(pipe)
            for k in ALL:
                assert_bits_equal(again[k].view(np.uint32), got[k].view(np.uint32), f"{what} second encode: {k}")
        finally:
            pipe.destroy()
    assert nan_pixels > 0, "the non-finite scenes are there for their NaN pixels"


def test_lists_that_end_at_the_chunk_edges(hip_device):
    """Tile lists of 1, 63, 64, 65, 128 and 129 entries (test_gpu_nan.chunk_edge_scene), none of which saturates a pixel: the walk's chunks of 64 end with
    the list, one entry before it and one entry after it.  The weight sum is the rasterizer's bit for bit, the expected depth within the float64 bound, and the median a record's z (here 0: no weight sum reaches one half)."""
    cfg, g, sh, cam = chunk_edge_scene()
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        got = _depth(pipe)
        fw = pipe.collect_forward()
        lens = tile_list_lengths(fw["tile_ranges"])
        ntx = (cfg.width + 15) // 16
        assert {t: int(lens[t[1] * ntx + t[0]]) for t in CHUNK_EDGE_PILES} == CHUNK_EDGE_PILES, "the scene is not the one this test is about"
        assert _assert_weight_sum_is_alpha(pipe, got, "chunk edges") == 0
        assert got["weight_sum"].max() < 0.99, "no pixel is to saturate: every chunk is walked to its end"
        A, D, M, near_sat, near_half, stats = depth64_of(fw, cfg, probe=got["median"])
        # expected depth, test_depth_images_match_float64's bound: the z kept beside each record, through every chunk of the list
        zmax = float(np.abs(d64.decode_depths(fw["depths"])[fw["sorted_values"]]).max())
        tol = (stats["n_active"] + 32) * 2.0 ** -23
        err = np.abs(got["expected"].astype(np.float64) - D) / zmax
        keep = ~near_sat
        print(f"depth accuracy chunk edges: worst share of the bound (n_p + 32) 2^-23 = {(err / tol)[keep].max():.3f}, max n_p = {int(stats['n_active'].max())}")
        assert int(stats["n_active"].max()) > 0 and np.all(err[keep] <= tol[keep]), f"chunk edges: expected depth off by {(err / tol)[keep].max():.2f} x the bound"
        assert np.all(got["expected"][stats["n_active"] == 0] == 0)
        sure = ~(near_sat | near_half)
        assert_bits_equal(got["median"][sure], M.astype(np.float32)[sure], "chunk edges: median depth")
        assert np.all(stats["probe_in_box"][(got["median"] != 0)]), "chunk edges: a median that is no record's z"
    finally:
        pipe.destroy()


def test_rerun_and_replay(hip_device):
    dev = hip_device
    cfg = scene_config("c2-20k")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        first = _depth(pipe)
        second = _depth(pipe)
        with dev.createCommandEncoder("depth", record=True) as enc:
            pipe.fwd.encode(enc)
            pipe.rast.encode(enc, cfg.width, cfg.height)
            pipe.rast.encodeDepth(enc, ALL)
            cmd = enc.finish()
        for k in ALL:
            assert_bits_equal(second[k], first[k], f"second eager encode: {k}")
            pipe.rast.getDepthTextureView(k).clear()
        dev.queue.submit([cmd])
        dev.synchronize()
        once = _read(pipe)
        dev.queue.submit([cmd])
        dev.synchronize()
        twice = _read(pipe)
        cmd.destroy()
        for k in ALL:
            assert_bits_equal(once[k], first[k], f"replayed recording: {k}")
            assert_bits_equal(twice[k], first[k], f"recording submitted twice: {k}")
    finally:
        pipe.destroy()


def test_only_the_kinds_asked_for_are_written(hip_device):
    cfg = scene_config("odd-size")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        full = _depth(pipe)
        for k in ALL:
            pipe.rast.getDepthTextureView(k).clear()
        only = _depth(pipe, ("median",))
        assert_bits_equal(only["median"], full["median"], "median alone")
        with pytest.raises(_lib.StateError):
            pipe.rast.getDepthTextureView("expected")
        pipe.rast.encodeDepth(None, 7)
        hip_device.synchronize()
        assert_bits_equal(_read(pipe)["expected"], full["expected"], "all three by mask")
        pipe.rast.encodeDepth(None, "weight_sum")
        hip_device.synchronize()
        assert_bits_equal(_read(pipe, ("weight_sum",))["weight_sum"], full["weight_sum"], "one kind given as a string")
    finally:
        pipe.destroy()


def test_encoding_depth_changes_nothing_else(hip_device):
    cfg = scene_config("c2-20k")
    g, sh, cam = harness.scene(cfg)
    a = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    b = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        a.forward()
        plain = a.collect_forward()
        _depth(b)
        with_depth = b.collect_forward()
        for k in ("rgba8", "final_T", "n_contrib", "sorted_keys", "sorted_values", "tile_ranges", "splats", "depths"):
            assert_bits_equal(with_depth[k], plain[k], f"frame with encodeDepth: {k}")
    finally:
        a.destroy()
        b.destroy()


def _trajectory(dev, cfg, g, sh, cameras, imgs, depth, with_viewer):
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False, pipeline_depth=depth)
    v = None
    if with_viewer:
        v = Viewer(dev, cfg.width, cfg.height)
        v.setCamera(cameras[1]["camera"])
        v.setPointCloud(t.pointCloud)
    try:
        for i in range(20):
            t.step()
            if v is not None:
                d = v.renderDepth("expected" if i % 2 else "median")
                assert d.shape == (cfg.height, cfg.width) and np.isfinite(d).all() and (d > 0).any()
        t.drain()
        st = t.optimizer.getStateBuffers()
        return dict(g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32), **{k: st[k].read(np.uint32) for k in st})
    finally:
        if v is not None:
            v.destroy()
        t.destroy()


@pytest.mark.parametrize("depth", [1, 2])
def test_trainer_trajectory_is_untouched_by_render_depth(hip_device, depth):
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(hip_device, cfg, 4)
    plain = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, False)
    watched = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, True)
    for k in plain:
        assert_bits_equal(watched[k], plain[k], f"20 steps with renderDepth between them, pipeline depth {depth}: {k}")


def test_state_errors(hip_device):
    dev = hip_device
    cfg = scene_config("sparse")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeDepth(None)            # nothing encoded at all
        pipe.fwd.encode(None)
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeDepth(None)            # the forward pass alone
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.getDepthTextureView("expected")
        with pytest.raises(_lib.WdgsError) as e:
            pipe.rast.encodeDepth(None, 0)
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.WdgsError) as e:
            pipe.rast.encodeDepth(None, 8)
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(ValueError):
            pipe.rast.encodeDepth(None, ("mean",))
        with pytest.raises(_lib.StateError):       # first use of a kind allocates its image: refused inside a recording
            with dev.createCommandEncoder("doomed", record=True) as enc:
                pipe.rast.encodeDepth(enc, ("expected",))
        dev.synchronize()
        pipe.rast.encodeDepth(None, ("expected",))
        with pytest.raises(_lib.StateError):
            pipe.rast.getDepthTextureView("median")
        with pytest.raises(_lib.StateError):       # another kind is a first use again
            with dev.createCommandEncoder("doomed", record=True) as enc:
                pipe.rast.encodeDepth(enc, ("expected", "median"))
        dev.synchronize()
        with dev.createCommandEncoder("fine", record=True) as enc:
            pipe.rast.encodeDepth(enc, ("expected",))
            enc.finish().destroy()
        pipe.fwd.setRenderMode("pointcloud")
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeDepth(None, ("expected",))
        pipe.fwd.setRenderMode("gaussian")
        got = _depth(pipe, ("expected",))
        assert (got["expected"] > 0).any()
    finally:
        pipe.destroy()


@pytest.mark.parametrize("name", ["c1", "big-splats", "sparse"])
def test_depth_to_rgba8(hip_device, name):
    dev = hip_device
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        d = _depth(pipe, ("expected",))["expected"]
        out = dev.createBuffer(4 * cfg.width * cfg.height)
        for near, far in ((float(d[d > 0].min()), float(d[d > 0].max())), (3.0, 7.5)):
            ops.depthToRGBA8(dev, pipe.rast.getDepthTextureView("expected"), cfg.width, cfg.height, near, far, out)
            rgba = out.read(np.uint8).reshape(cfg.height, cfg.width, 4)
            want, v = d64.depth_to_rgba8_64(d, near, far)
            assert np.all(rgba[..., 3] == 255) and np.array_equal(rgba[..., 0], rgba[..., 1]) and np.array_equal(rgba[..., 0], rgba[..., 2])
            assert np.all(rgba[..., 0][d == 0] == 0)
            ties = np.abs((v - np.floor(v)) - 0.5) < 1e-3
            diff = np.abs(rgba[..., 0].astype(np.int32) - want.astype(np.int32))
            print(f"depth_to_rgba8 {name} [{near:.3g}, {far:.3g}]: ties {ties.mean():.4%}, pixels off by one {np.mean(diff == 1):.4%}")
            assert ties.mean() <= 0.005
            assert np.all(diff[~ties] == 0) and np.all(diff <= 1)
        for bad in ((0.0, 1.0), (2.0, 2.0), (3.0, 1.0), (1.0, float("inf"))):
            with pytest.raises(_lib.WdgsError):
                ops.depthToRGBA8(dev, pipe.rast.getDepthTextureView("expected"), cfg.width, cfg.height, bad[0], bad[1], out)
        out.destroy()
    finally:
        pipe.destroy()


def test_viewer_render_depth_end_to_end(hip_device, tmp_path):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20_000, width=320, height=240)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8)[3]
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    v = Viewer(dev, cfg.width, cfg.height)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        v.setCamera(cam)
        v.setPointCloud(pc)                      # starts in point-cloud mode
        v.render(None)
        before = v.readFrame().copy()
        med = v.renderDepth("median")
        assert v._settings["renderMode"] == "pointcloud"
        assert med.dtype == np.float32 and med.shape == (cfg.height, cfg.width)
        assert_bits_equal(med, _depth(pipe, ("median",))["median"], "Viewer.renderDepth vs encodeDepth on a pipeline with the same camera")
        v.render(None)
        assert_bits_equal(v.readFrame(), before, "the frame after renderDepth")
        # back-projection: each point, taken through the view matrix again, lies at the image's depth
        pts = loaders.backprojectDepth(med, cam)
        ys, xs = np.nonzero(med > 0)
        assert len(pts) == len(ys) > med.size // 2   # (a median needs a weight sum of one half: most of this scene, not all)
        view = cam[0:16].astype(np.float64).reshape(4, 4).T
        vz = (np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], axis=1) @ view.T)[:, 2]
        # (the bound of tests/test_depth_reference.py: 20 m^2 2^-24 s, m = the matrices' largest entry, s = the points' largest coordinate)
        m = max(1.0, np.abs(cam[0:32]).max())
        bound = 20.0 * m * m * 2.0 ** -24 * max(np.abs(pts).max(), np.abs(med).max())
        assert np.abs(vz - med[ys, xs]).max() <= bound
        # gaussian mode: the same image, and the mode stays
        v.setRenderMode("gaussian")
        assert_bits_equal(v.renderDepth("median"), med, "renderDepth in gaussian mode")
        assert v._settings["renderMode"] == "gaussian"
        exp = v.renderDepth()
        path = str(tmp_path / "depth.png")
        v.saveDepthPNG(path)
        with open(path, "rb") as f:
            png = images.decodePNG(f.read())
        want, tv = d64.depth_to_rgba8_64(exp, exp[exp > 0].min(), exp[exp > 0].max())
        ties = np.abs((tv - np.floor(tv)) - 0.5) < 1e-3
        assert png.shape == (cfg.height, cfg.width, 4) and np.all(png[..., 3] == 255)
        assert np.all(png[..., 0][~ties] == want[~ties]) and png[..., 0].max() == 255
    finally:
        pipe.destroy()
        v.destroy()
