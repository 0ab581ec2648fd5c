"""GPU: the normal maps (csrc/normal.hip).  The per-Gaussian words and the composited image against the float64 restatement
(tests/normal64.py), the weight channel against depth's weight_sum and the alpha texture bit for bit, determinism and recording, that normals change
nothing else, state errors, the three image kernels (depth normals, agreement, presentation), and the Viewer / Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, images, ops, synth
from webdgs_amd.viewer import Viewer

import harness
import normal64 as n64
from harness import assert_bits_equal
from test_depth_reference import MASK_CAP, SCENES, scene_config
from test_gpu_depth import _special_scenes
from test_gpu_eval import _trainer, _views
from test_gpu_nan import CHUNK_EDGE_PILES, INF16, NAN16, chunk_edge_scene, tile_list_lengths
from test_normal_reference import PLANES, _plane_depth

pytestmark = pytest.mark.gpu

U = n64.U
# The float64 walk is taken three times per image (once per component).  A scene too large for one case of a few seconds is split over several cases,
# part k of n walking the tiles t with t % n == k: together they walk every tile, and every case checks the bit-level identities on all pixels.
PARTS = {"c2": 7}
WHOLE_BELOW = 100_000     # tile entries an unsplit scene may have (a scene that outgrows it belongs in PARTS)


def _read(pipe):
    cfg = pipe.cfg
    words = pipe.rast.getGaussianNormals().read(np.uint32)[:cfg.num_points].copy()
    img = pipe.rast.getNormalTextureView().read(np.float32).reshape(cfg.height, cfg.width, 4).copy()
    return words, img


def _normals(pipe):
    pipe.forward()
    pipe.rast.encodeNormal(None)
    pipe.dev.synchronize()
    return _read(pipe)


def _assert_weight_channel(pipe, img, what):
    """A against encodeDepth's weight_sum (bits; NaN pixels NaN in both) and 1.0f - A against the alpha texture.  Returns the number of NaN pixels."""
    cfg = pipe.cfg
    pipe.rast.encodeDepth(None, ("weight_sum",))
    pipe.dev.synchronize()
    ws = pipe.rast.getDepthTextureView("weight_sum").read(np.float32).reshape(cfg.height, cfg.width)
    alpha = pipe.rast.getAlphaTextureView().read(np.float32).reshape(cfg.height, cfg.width)
    A = img[..., 3]
    nan = np.isnan(ws)
    assert np.array_equal(nan, np.isnan(A)) and np.array_equal(nan, np.isnan(alpha)), f"{what}: NaN pixels differ"
    assert_bits_equal(np.where(nan, np.float32(0), A), np.where(nan, np.float32(0), ws), f"{what}: A vs depth's weight_sum")
    with np.errstate(invalid="ignore"):
        mine = np.float32(1) - A
    assert_bits_equal(np.where(nan, np.float32(0), mine), np.where(nan, np.float32(0), alpha), f"{what}: 1 - A vs the alpha texture")
    return int(nan.sum())


def _assert_image_matches_float64(pipe, words, img, what, max_entries=0, part=(0, 1)):
    """The composited normal against normal64 fed with the GPU's own forward stages and its own packed words.  Per component: one rounding per FMA and
    a few ulp of the deterministic exp on the weights that matter, on values of size <= 1 -- depth's bound with max|z| = 1 -- the decode being shared
    (ops.decodeNormals is the kernel's, operation by operation): (n_p + 32) 2^-23."""
    cfg = pipe.cfg
    fw = pipe.collect_forward()
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    k, parts = part
    assert parts > 1 or fw["total_entries"] <= WHOLE_BELOW, fw["total_entries"]
    tiles = None if parts == 1 else (np.arange(int(ti[2])) % parts == k)
    A, N, near_sat, n_active = n64.composite64(st, ti, fw, ops.decodeNormals(words), max_entries=max_entries, tiles=tiles)
    walked = np.ones(A.shape, bool) if tiles is None else n64.tile_pixels(tiles, cfg.width, cfg.height)
    assert near_sat[walked].mean() <= MASK_CAP, near_sat[walked].mean()
    keep = walked & ~near_sat
    tol = (n_active + 32) * 2.0 ** -23
    err = np.abs(img[..., :3].astype(np.float64) - N).max(axis=2)
    share = (err / tol)[keep].max()
    print(f"normal accuracy {what}: max |N - N64| = {err[keep].max():.3e}, worst share of the bound (n_p + 32) 2^-23 = {share:.3f}, max n_p = {int(n_active[keep].max())}, "
          f"near_sat {near_sat[walked].mean():.4%}, E = {fw['total_entries']}, tiles {k} mod {parts}")
    assert np.all(err[keep] <= tol[keep]), f"{what}: composited normal off by {share:.2f} x the bound"
    assert np.abs(img[..., 3].astype(np.float64) - A)[keep].max() <= 1e-6
    assert np.all(img[..., :3][walked & (n_active == 0)] == 0)
    length = np.linalg.norm(img[..., :3].astype(np.float64), axis=2)
    assert np.all(length[keep] <= img[..., 3][keep] * (1 + 4 * U) + tol[keep]), f"{what}: |N| <= A"
    return n_active


# ---------------------------------------------------------------- 1. the per-Gaussian words
def _assert_words_match_float64(words, g, cam, what):
    ref = n64.gaussian_normals64(g, cam)
    assert np.array_equal(words == np.uint32(n64.NO_NORMAL), ~ref["valid"]), f"{what}: which Gaussians have no normal"
    v = ref["valid"]
    dec = ops.decodeNormals(words).astype(np.float64)
    near_flip = v & (np.abs(ref["facing"]) < n64.NEAR_FLIP)
    same = np.linalg.norm(dec - ref["normal"], axis=1)
    other = np.linalg.norm(dec + ref["normal"], axis=1)
    assert near_flip.mean() <= 0.005
    sure = v & ~near_flip
    print(f"gaussian normals {what}: worst |n - n64| = {same[sure].max():.3e} = {same[sure].max() / n64.WORD_BOUND:.3f} of the bound {n64.WORD_BOUND:.3e}; "
          f"near_flip {near_flip.mean():.4%}, of which turned the other way {int((other[near_flip] < same[near_flip]).sum())}")
    assert np.all(same[sure] <= n64.WORD_BOUND), f"{what}: {same[sure].max() / n64.WORD_BOUND:.2f} x the bound (or a flip outside the mask)"
    assert np.all(np.minimum(same, other)[near_flip] <= n64.WORD_BOUND), f"{what}: inside the mask the normal is + or - the float64 one"
    assert np.all(np.abs(np.linalg.norm(dec[v], axis=1) - 1) <= 4 * U)
    return ref


@pytest.mark.parametrize("name,view", [("c1", "identity"), ("c1", "circle"), ("big-splats", "identity"), ("sparse", "identity")])
def test_gaussian_words_match_float64(hip_device, name, view):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    if view == "circle":
        cam = synth.circle_cameras(cfg, 8)[3]
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        words, _ = _normals(pipe)
        _assert_words_match_float64(words, g, cam, f"{name} {view}")
    finally:
        pipe.destroy()


def _crafted_records():
    """Rows (12 halves) with a known answer, all at (1, 1, 4) under the identity camera, where every axis faces away and is turned round."""
    f16 = lambda v: np.float16(v).view(np.uint16)   # noqa: E731
    rows, want = [], []

    def add(q=(1, 0, 0, 0), ls=(-3, -2, -2), pos=(1.0, 1.0, 4.0), opacity=0.5, expect=None):
        r = np.zeros(12, np.uint16)
        r[0:3] = [f16(v) if not isinstance(v, int) else v for v in pos]
        r[3] = f16(opacity) if not isinstance(opacity, int) else opacity
        r[4:8] = [f16(v) if not isinstance(v, int) or abs(v) <= 2 else v for v in q]
        r[8:11] = [f16(v) if not isinstance(v, int) or abs(v) <= 8 else v for v in ls]
        rows.append(r)
        want.append(expect)

    add(ls=(-3, -2, -2), expect=(-1, 0, 0))
    add(ls=(-2, -3, -2), expect=(0, -1, 0))
    add(ls=(-2, -2, -3), expect=(0, 0, -1))
    add(ls=(-2, -3, -3), expect=(0, -1, 0))          # a two-way tie: the lower index
    add(ls=(-3, -2, -3), expect=(-1, 0, 0))
    add(ls=(-3, -3, -3), expect=(-1, 0, 0))          # a three-way tie
    add(ls=(0.0, -0.0, 1.0), expect=(-1, 0, 0))      # +0 and -0 are equal
    add(pos=(-1.0, -1.0, 4.0), ls=(-3, -2, -2), expect=(1, 0, 0))   # ... and from the other side e_x already faces the camera
    add(q=(0, 0, 0, 0), expect=None)                 # zero quaternion
    for bad in (NAN16, INF16, 0xFE00, 0xFC00):
        add(q=(1, bad, 0, 0), expect=None)
        add(ls=(-3, bad, -2), expect=None)
        add(pos=(1.0, bad, 4.0), expect=None)
    add(opacity=NAN16, expect=(-1, 0, 0))            # the opacity does not count
    add(q=(2, 0, 0, 0), ls=(-2, -2, -3), expect=(0, 0, -1))   # not unit: normalised
    return np.stack(rows), want


@pytest.mark.parametrize("n", [1, 257, 300])
def test_crafted_records_and_partial_workgroups(hip_device, n):
    cfg0 = scene_config("sparse")
    g0, sh0, cam = harness.scene(cfg0)
    rows, want = _crafted_records()
    gh = g0.view(np.uint16).reshape(-1, 12).copy()
    # q against 2 q (exact in fp16): rows 40.. hold the doubled quaternions of rows 0..39 of the scene
    gh[40:80] = gh[0:40]
    gh[40:80, 4:8] = (gh[0:40, 4:8].view(np.float16).astype(np.float32) * 2).astype(np.float16).view(np.uint16)
    k = len(rows)
    gh[100:100 + k] = rows
    gh = np.roll(gh, -100, axis=0) if n == 1 else gh     # (n = 1: the first crafted record alone)
    g = np.ascontiguousarray(gh[:n]).view(np.uint32).reshape(n, 6)
    cfg = harness.small_config("c1", num_points=n)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh0[:n], cam)
    try:
        words, img = _normals(pipe)
        assert words.shape == (n,)
        _assert_words_match_float64(words, g, cam, f"crafted, {n} points")
        dec = ops.decodeNormals(words)
        first = 0 if n == 1 else 100
        for i, w in enumerate(want[:max(0, min(k, n - first))]):
            if w is None:
                assert words[first + i] == n64.NO_NORMAL, f"crafted record {i}: {words[first + i]:#x}"
            else:
                assert np.array_equal(dec[first + i], np.array(w, np.float32)), f"crafted record {i}: {dec[first + i]} vs {w}"
        if n > 80:
            d = np.linalg.norm(dec[40:80].astype(np.float64) - dec[0:40].astype(np.float64), axis=1)
            print(f"2q against q: worst difference {d.max():.3e} (bound {n64.WORD_BOUND:.3e}); identical words: {int((words[40:80] == words[0:40]).sum())} of 40")
            assert np.all(d <= n64.WORD_BOUND)
        assert not np.any(words[np.setdiff1d(np.arange(n), first + np.array([i for i, w in enumerate(want) if w is None]))] == n64.NO_NORMAL)
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- 2. the composited image
@pytest.mark.parametrize("compat", [False, True], ids=["uncapped", "compatCaps"])
@pytest.mark.parametrize("name,part", [(name, (k, PARTS.get(name, 1))) for name in SCENES for k in range(PARTS.get(name, 1))],
                         ids=[name + (f"-tiles{k}of{PARTS[name]}" if name in PARTS else "") for name in SCENES for k in range(PARTS.get(name, 1))])
def test_composited_image_matches_float64(hip_device, name, part, compat):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam, compat_caps=compat)
    try:
        words, img = _normals(pipe)
        assert _assert_weight_channel(pipe, img, name) == 0
        _assert_image_matches_float64(pipe, words, img, f"{name} compat={compat}", max_entries=8192 if compat else 0, part=part)
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- 3. chunk edges
def test_lists_that_end_at_the_chunk_edges(hip_device):
    cfg, g, sh, cam = chunk_edge_scene()
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    try:
        words, img = _normals(pipe)
        fw = pipe.collect_forward()
        lens = tile_list_lengths(fw["tile_ranges"])
        ntx = (cfg.width + 15) // 16
        assert {t: int(lens[t[1] * ntx + t[0]]) for t in CHUNK_EDGE_PILES} == CHUNK_EDGE_PILES, "the scene is not the one this test is about"
        assert _assert_weight_channel(pipe, img, "chunk edges") == 0
        assert img[..., 3].max() < 0.99, "no pixel is to saturate: every chunk is walked to its end"
        n_active = _assert_image_matches_float64(pipe, words, img, "chunk edges")
        assert int(n_active.max()) > 0
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- 4. long lists, non-finite scenes, Gaussians without a normal
@pytest.mark.parametrize("compat", [False, True], ids=["uncapped", "compatCaps"])
def test_long_lists_and_non_finite_scenes(hip_device, compat):
    nan_pixels = no_normal = 0
    for what, cfg, g, sh, cam in _special_scenes():
        pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam, compat_caps=compat)
        try:
            words, img = _normals(pipe)
            nan_pixels += _assert_weight_channel(pipe, img, what)
            ref = n64.gaussian_normals64(g, cam)
            assert np.array_equal(words == np.uint32(n64.NO_NORMAL), ~ref["valid"]), what
            no_normal += int((~ref["valid"]).sum())
            words2, img2 = _normals(pipe)
            assert_bits_equal(words2, words, f"{what} second encode: words")
            assert_bits_equal(img2.view(np.uint32), img.view(np.uint32), f"{what} second encode: image")
        finally:
            pipe.destroy()
    assert nan_pixels > 0 and no_normal > 0, "the non-finite scenes are there for their NaN pixels and their Gaussians without a normal"


def test_a_gaussian_without_a_normal_adds_weight_and_no_normal(hip_device):
    """Zero quaternions: R(0) is the identity, so the Gaussian is projected and composited as ever, and has no normal."""
    cfg = scene_config("big-splats")
    g, sh, cam = harness.scene(cfg)
    for every in (1, 2):
        gh = g.view(np.uint16).reshape(-1, 12).copy()
        gh[::every, 4:8] = 0
        gz = gh.view(np.uint32).reshape(-1, 6)
        pipe = harness.HipPipeline(hip_device, cfg, gz, sh, cam)
        try:
            words, img = _normals(pipe)
            assert np.all(words[::every] == n64.NO_NORMAL) and (every == 1 or not np.any(words[1::2] == n64.NO_NORMAL))
            assert _assert_weight_channel(pipe, img, f"every {every}") == 0
            assert (img[..., 3] > 0.5).mean() > 0.5
            if every == 1:
                assert np.all(img[..., :3] == 0), "no Gaussian has a normal: N is zero wherever A is not"
            else:
                _assert_image_matches_float64(pipe, words, img, "every second Gaussian without a normal")
        finally:
            pipe.destroy()


# ---------------------------------------------------------------- 5. rerun and replay
def test_rerun_and_replay(hip_device):
    dev = hip_device
    cfg = scene_config("c2-20k")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        pipe.forward()
        with pytest.raises(_lib.StateError):       # first use allocates: refused inside a recording
            with dev.createCommandEncoder("doomed", record=True) as enc:
                pipe.rast.encodeNormal(enc)
        dev.synchronize()
        w1, i1 = _normals(pipe)
        w2, i2 = _normals(pipe)
        assert_bits_equal(w2, w1, "second eager encode: words")
        assert_bits_equal(i2, i1, "second eager encode: image")
        with dev.createCommandEncoder("normal", record=True) as enc:
            pipe.fwd.encode(enc)
            pipe.rast.encode(enc, cfg.width, cfg.height)
            pipe.rast.encodeNormal(enc)
            cmd = enc.finish()
        for round_ in ("replayed recording", "recording submitted twice"):
            pipe.rast.getNormalTextureView().clear()
            pipe.rast.getGaussianNormals().clear()
            dev.queue.submit([cmd])
            dev.synchronize()
            w, i = _read(pipe)
            assert_bits_equal(w, w1, f"{round_}: words")
            assert_bits_equal(i, i1, f"{round_}: image")
        cmd.destroy()
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- 6. normals change nothing else
def test_encoding_normals_changes_nothing_else(hip_device):
    cfg = scene_config("c2-20k")
    g, sh, cam = harness.scene(cfg)
    a = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    b = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    kinds = ("expected", "median", "weight_sum")
    stats_a, stats_b = ops.createContributionBuffer(hip_device, cfg.num_points), ops.createContributionBuffer(hip_device, cfg.num_points)
    try:
        a.forward()
        a.rast.encodeDepth(None, kinds)
        a.rast.encodeContribution(None, stats_a)
        hip_device.synchronize()
        plain = a.collect_forward()
        b.forward()
        b.rast.encodeNormal(None)
        b.rast.encodeDepth(None, kinds)
        b.rast.encodeNormal(None)
        b.rast.encodeContribution(None, stats_b)
        b.rast.encodeNormal(None)
        hip_device.synchronize()
        with_normals = b.collect_forward()
        for k in ("rgba8", "final_T", "n_contrib", "sorted_keys", "sorted_values", "tile_ranges", "splats", "depths"):
            assert_bits_equal(with_normals[k], plain[k], f"frame with encodeNormal: {k}")
        for k in kinds:
            assert_bits_equal(b.rast.getDepthTextureView(k).read(np.uint32), a.rast.getDepthTextureView(k).read(np.uint32), f"depth image {k}")
        assert_bits_equal(stats_b.read(np.uint8), stats_a.read(np.uint8), "contribution records")
        assert_bits_equal(b.pc.gaussian_3d_buffer.read(np.uint32), a.pc.gaussian_3d_buffer.read(np.uint32), "the cloud")
        assert_bits_equal(b.camera.read(np.uint32), a.camera.read(np.uint32), "the camera block")
    finally:
        stats_a.destroy()
        stats_b.destroy()
        a.destroy()
        b.destroy()


def _trajectory(dev, cfg, g, sh, cameras, imgs, depth, watched):
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False, pipeline_depth=depth)
    v = None
    if watched:
        v = Viewer(dev, cfg.width, cfg.height)
        v.setCamera(cameras[1]["camera"])
        v.setPointCloud(t.pointCloud)
    try:
        for i in range(20):
            t.step()
            if v is not None and i % 2:
                n = v.renderNormals()
                assert n.shape == (cfg.height, cfg.width, 4) and np.isfinite(n).all() and (n[..., 3] > 0).any()
            if watched and i % 5 == 2:
                r = t.normalConsistency([i % 4], split="train", depthKind="expected" if i % 2 else "median")
                assert r["pixels"][0] > 0 and 0.0 <= r["mean"] <= 2.0
        t.drain()
        st = t.optimizer.getStateBuffers()
        return dict(g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32), rng=np.array(t._rng.getstate()[1]),
                    **{k: st[k].read(np.uint32) for k in st})
    finally:
        if v is not None:
            v.destroy()
        t.destroy()


@pytest.mark.parametrize("depth", [1, 2])
def test_trainer_trajectory_is_untouched_by_normals(hip_device, depth):
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(hip_device, cfg, 4)
    plain = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, False)
    watched = _trajectory(hip_device, cfg, g, sh, cameras, imgs, depth, True)
    for k in plain:
        assert_bits_equal(watched[k], plain[k], f"20 steps with renderNormals and normalConsistency between them, pipeline depth {depth}: {k}")


# ---------------------------------------------------------------- 7. state errors
def test_state_errors(hip_device):
    dev = hip_device
    cfg = scene_config("sparse")
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    n = cfg.width * cfg.height
    img, dn, out8, sums, depth = dev.createBuffer(16 * n), dev.createBuffer(16 * n), dev.createBuffer(4 * n), dev.createBuffer(24), dev.createBuffer(4 * n)
    try:
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeNormal(None)            # nothing encoded at all
        pipe.fwd.encode(None)
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeNormal(None)            # the forward pass alone
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.getNormalTextureView()        # the getters before their encoder
        with pytest.raises(_lib.StateError):
            pipe.rast.getGaussianNormals()
        pipe.fwd.setRenderMode("pointcloud")
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.encodeNormal(None)            # point-cloud mode has no weights
        pipe.fwd.setRenderMode("gaussian")
        words, image = _normals(pipe)
        assert (image[..., 3] > 0).any() and not np.any(words == n64.NO_NORMAL)
        lib, h = dev.lib, dev.handle
        rast = pipe.rast.handle
        for code in (lib.wdgs_tiled_rasterizer_encode_normal(rast, None, pipe.camera.ptr), lib.wdgs_tiled_rasterizer_encode_normal(rast, pipe.pc.gaussian_3d_buffer.ptr, None),
                     lib.wdgs_tiled_rasterizer_encode_normal(None, pipe.pc.gaussian_3d_buffer.ptr, pipe.camera.ptr),
                     lib.wdgs_tiled_rasterizer_get_normal(rast, None), lib.wdgs_tiled_rasterizer_get_gaussian_normals(None, None),
                     # null arguments and bad sizes of the three image kernels
                     lib.wdgs_depth_to_normals(h, None, cfg.width, cfg.height, 1.0, -1.0, dn.ptr), lib.wdgs_depth_to_normals(h, depth.ptr, cfg.width, cfg.height, 1.0, -1.0, None),
                     lib.wdgs_depth_to_normals(None, depth.ptr, cfg.width, cfg.height, 1.0, -1.0, dn.ptr), lib.wdgs_depth_to_normals(h, depth.ptr, 0, cfg.height, 1.0, -1.0, dn.ptr),
                     lib.wdgs_depth_to_normals(h, depth.ptr, cfg.width, 0, 1.0, -1.0, dn.ptr), lib.wdgs_depth_to_normals(h, depth.ptr, 65536, 65536, 1.0, -1.0, dn.ptr),
                     lib.wdgs_depth_to_normals(h, depth.ptr, cfg.width, cfg.height, 0.0, -1.0, dn.ptr), lib.wdgs_depth_to_normals(h, depth.ptr, cfg.width, cfg.height, 1.0, float("nan"), dn.ptr),
                     lib.wdgs_depth_to_normals(h, depth.ptr, cfg.width, cfg.height, float("inf"), -1.0, dn.ptr),
                     lib.wdgs_normal_agreement(h, None, dn.ptr, cfg.width, cfg.height, sums.ptr), lib.wdgs_normal_agreement(h, img.ptr, None, cfg.width, cfg.height, sums.ptr),
                     lib.wdgs_normal_agreement(h, img.ptr, dn.ptr, cfg.width, cfg.height, None), lib.wdgs_normal_agreement(h, img.ptr, dn.ptr, 0, 1, sums.ptr),
                     lib.wdgs_normal_agreement(h, img.ptr, dn.ptr, 65536, 65536, sums.ptr), lib.wdgs_normal_agreement(h, img.ptr + 4, dn.ptr, 8, 8, sums.ptr),
                     lib.wdgs_normal_to_rgba8(h, None, cfg.width, cfg.height, out8.ptr), lib.wdgs_normal_to_rgba8(h, img.ptr, cfg.width, cfg.height, None),
                     lib.wdgs_normal_to_rgba8(h, img.ptr, 0, 0, out8.ptr), lib.wdgs_normal_to_rgba8(h, img.ptr, 65536, 32768, out8.ptr)):
            assert code == _lib.WDGS_E_INVALID
        for call in (lambda: ops.depthToNormals(dev, depth, cfg.width + 1, cfg.height, cam, dn), lambda: ops.normalToRGBA8(dev, img, cfg.width, cfg.height + 1, out8),
                     lambda: ops.normalAgreement(dev, img, out8, cfg.width, cfg.height)):
            with pytest.raises(ValueError):
                call()
        # a change of the point count re-makes the words: refused inside a recording, fine eagerly
        pipe.pc2 = ops.createPointCloud(dev, g[:100], sh[:100], cfg.sh_deg)
        assert pipe.fwd.setPointCloud(pipe.pc2)
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.getGaussianNormals()          # the words of another point count
        with pytest.raises(_lib.StateError):
            with dev.createCommandEncoder("doomed", record=True) as enc:
                pipe.rast.encodeNormal(enc)
        dev.synchronize()
        pipe.rast.encodeNormal(None)
        dev.synchronize()
        assert_bits_equal(pipe.rast.getGaussianNormals().read(np.uint32)[:100], words[:100], "the first 100 Gaussians' words after the cloud shrank")
        with dev.createCommandEncoder("fine", record=True) as enc:
            pipe.rast.encodeNormal(enc)
            enc.finish().destroy()
        # ... and a larger cloud: the words of the smaller one are not handed out (they hold 100 Gaussians, the getter's view would span 300)
        assert pipe.fwd.setPointCloud(pipe.pc)
        with pytest.raises(_lib.StateError):
            pipe.rast.getGaussianNormals()
        pipe.forward()
        with pytest.raises(_lib.StateError):
            pipe.rast.getGaussianNormals()
        pipe.rast.getNormalTextureView()            # (the image has the size it had)
        w3, _ = _normals(pipe)
        assert_bits_equal(w3, words, "the words after the cloud grew back")
    finally:
        for b in (img, dn, out8, sums, depth):
            b.destroy()
        pipe.destroy()


# ---------------------------------------------------------------- 8. depthToNormals
def _depth_normals_gpu(dev, depth, cam):
    h, w = depth.shape
    src, dst = dev.bufferFrom(np.ascontiguousarray(depth, np.float32)), dev.createBuffer(16 * w * h)
    try:
        ops.depthToNormals(dev, src, w, h, cam, dst)
        return dst.read(np.float32).reshape(h, w, 4).copy()
    finally:
        src.destroy()
        dst.destroy()


def _assert_depth_normals(got, depth_f32, cam, what, eps=1e-4):
    """Against the float64 stencil of the same f32 image, within the per-pixel f32 bound (normal64.depth_normals_f32_bound).  Pixels whose float64 cross
    product is shorter than `eps` Z (|a| + |b|) -- the two differences all but parallel, or both all but zero, so that the bound says nothing -- are
    left out, at most MASK_CAP of the image."""
    dn = n64.depth_normals64(depth_f32, cam[32], cam[37])
    short = dn["valid"] & (dn["cross"] < eps * dn["zmax"] * (dn["a"] + dn["b"]))
    assert short.mean() <= MASK_CAP, f"{what}: {short.mean():.3%} of the pixels have a short cross product"
    keep = ~short
    assert np.array_equal((got[..., 3] != 0)[keep], dn["valid"][keep]), f"{what}: which pixels have a normal"
    assert np.all(got[~dn["valid"] & keep] == 0) and np.all(got[..., 3][dn["valid"] & keep] == 1)
    bound = n64.depth_normals_f32_bound(dn)
    err = np.linalg.norm(got[..., :3].astype(np.float64) - dn["normal"], axis=2)
    ok = dn["valid"] & keep
    share = (err[ok] / bound[ok]).max() if ok.any() else 0.0
    print(f"depth normals {what}: {ok.mean():.1%} of the pixels valid, worst |n - n64| = {err[ok].max() if ok.any() else 0:.3e}, worst share of the f32 bound {share:.3f}, "
          f"short cross products {short.mean():.4%}")
    assert np.all(err[ok] <= bound[ok]), f"{what}: off by {share:.2f} x the bound"
    return dn


@pytest.mark.parametrize("normal,dist", PLANES)
def test_depth_normals_of_analytic_planes(hip_device, normal, dist):
    cfg = harness.small_config("c1", num_points=1, width=97, height=61)
    cam = synth.identity_camera(cfg)
    z, want = _plane_depth(cfg.width, cfg.height, cam, normal, dist, np.float32)
    got = _depth_normals_gpu(hip_device, z, cam)
    dn = _assert_depth_normals(got, z, cam, f"plane {normal}")
    inner = np.zeros(z.shape, bool)
    inner[1:-1, 1:-1] = True
    assert np.array_equal(got[..., 3] == 1, inner) and np.all(got[~inner] == 0), "borders have no normal"
    # against the analytic normal: the same bound -- a coordinate takes four roundings in the kernel, and the bound's fifth u is the f32 depth's own
    err = np.linalg.norm(got[..., :3][inner].astype(np.float64) - want, axis=1)
    assert np.all(err <= n64.depth_normals_f32_bound(dn)[inner])
    holes = z.copy()
    holes[20, 30], holes[40, 50], holes[10, 10], holes[30, 60] = 0.0, -1.0, np.nan, np.inf
    gh = _depth_normals_gpu(hip_device, holes, cam)
    for (j, i) in ((20, 30), (40, 50), (10, 10), (30, 60)):
        for dj, di in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            assert np.all(gh[j + dj, i + di] == 0)
    assert int((gh[..., 3] == 1).sum()) == int(inner.sum()) - 20
    assert_bits_equal(gh[gh[..., 3] == 1], got[gh[..., 3] == 1], "pixels away from the holes")


@pytest.mark.parametrize("name", ["c1", "big-splats", "sparse"])
def test_depth_normals_of_a_scene(hip_device, name):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(hip_device, cfg, g, sh, cam)
    dst = hip_device.createBuffer(16 * cfg.width * cfg.height)
    try:
        pipe.forward()
        pipe.rast.encodeDepth(None, ("median", "expected"))
        for kind in ("median", "expected"):
            ops.depthToNormals(hip_device, pipe.rast.getDepthTextureView(kind), cfg.width, cfg.height, cam, dst)
            got = dst.read(np.float32).reshape(cfg.height, cfg.width, 4)
            d = pipe.rast.getDepthTextureView(kind).read(np.float32).reshape(cfg.height, cfg.width)
            dn = _assert_depth_normals(got, d, cam, f"{name} {kind}")
            assert dn["valid"].any()
            ops.depthToNormals(hip_device, pipe.rast.getDepthTextureView(kind), cfg.width, cfg.height, (cam[32], cam[37]), dst)
            assert_bits_equal(dst.read(np.float32).reshape(got.shape), got, "P00 and P11 given as a pair")
    finally:
        dst.destroy()
        pipe.destroy()


# ---------------------------------------------------------------- 9. normalAgreement
@pytest.mark.parametrize("name", ["c1", "big-splats", "sparse"])
def test_normal_agreement_matches_float64(hip_device, name):
    dev = hip_device
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    dst = dev.createBuffer(16 * cfg.width * cfg.height)
    try:
        words, img = _normals(pipe)
        pipe.rast.encodeDepth(None, ("median",))
        ops.depthToNormals(dev, pipe.rast.getDepthTextureView("median"), cfg.width, cfg.height, cam, dst)
        got = ops.normalAgreement(dev, pipe.rast.getNormalTextureView(), dst, cfg.width, cfg.height)
        e, a, cnt = n64.agreement64(img, dst.read(np.float32).reshape(cfg.height, cfg.width, 4))
        print(f"normal agreement {name}: {got['pixels']} pixels, 1 - cos = {got['value']:.6f}, |sum_e - float64| = {abs(got['sum_e'] - e)} "
              f"(bound {n64.AGREEMENT_UNITS_PER_PIXEL} per pixel = {n64.AGREEMENT_UNITS_PER_PIXEL * cnt})")
        assert got["pixels"] == cnt > 0 and got["sum_a"] == a
        assert abs(got["sum_e"] - e) <= n64.AGREEMENT_UNITS_PER_PIXEL * cnt
        assert got["value"] == got["sum_e"] / got["sum_a"] and 0 < got["value"] < 2
        again = ops.normalAgreement(dev, pipe.rast.getNormalTextureView(), dst, cfg.width, cfg.height)
        assert again == got, "integer sums: the same bytes every time"
    finally:
        dst.destroy()
        pipe.destroy()


def test_flat_grid_agrees_with_its_own_depth_exactly(hip_device):
    """Identity-quaternion Gaussians, flat in z, on a grid at view depth 4 (identity camera): every normal is (0, 0, -1) and every depth is 4, exactly."""
    dev = hip_device
    cfg0 = harness.small_config("c1", num_points=1, width=64, height=48, sh_deg=0, fy=64.0)
    rows = []
    for py in range(2, 48, 4):
        for px in range(2, 64, 4):
            r = np.zeros(12, np.float16)
            r[0:4] = [(px - 32) / 16.0, (py - 24) / 16.0, 4.0, 3.0]     # pixel = x fy / z + W / 2: multiples of 1/16 are fp16-exact
            r[4] = 1.0
            r[8:11] = [np.log(0.1875), np.log(0.1875), np.log(0.1875) - 2.0]
            rows.append(r)
    g = np.stack(rows).view(np.uint32).reshape(-1, 6)
    cfg = harness.small_config("c1", num_points=len(rows), width=64, height=48, sh_deg=0, fy=64.0)
    sh = np.zeros((len(rows), 24), np.uint32)
    cam = synth.identity_camera(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    dst = dev.createBuffer(16 * cfg.width * cfg.height)
    try:
        words, img = _normals(pipe)
        assert np.all(words == 0), "(0, 0, -1) is the centre of the octahedral square"
        A = img[..., 3]
        assert (A >= 0.5).mean() > 0.9
        assert np.all(img[..., 0] == 0) and np.all(img[..., 1] == 0)
        assert_bits_equal(img[..., 2], -A, "N_z = -A")
        pipe.rast.encodeDepth(None, ("expected",))
        d = pipe.rast.getDepthTextureView("expected").read(np.float32).reshape(cfg.height, cfg.width)
        assert np.all(d[A > 0] == 4.0) and np.all(d[A == 0] == 0)
        ops.depthToNormals(dev, pipe.rast.getDepthTextureView("expected"), cfg.width, cfg.height, cam, dst)
        dn = dst.read(np.float32).reshape(cfg.height, cfg.width, 4)
        has = A > 0
        inner = np.zeros(A.shape, bool)
        inner[1:-1, 1:-1] = has[1:-1, 1:-1] & has[1:-1, :-2] & has[1:-1, 2:] & has[:-2, 1:-1] & has[2:, 1:-1]
        assert inner.mean() > 0.8
        assert np.all(dn[inner] == np.array([0, 0, -1, 1], np.float32)) and np.all(dn[~inner] == 0)
        got = ops.normalAgreement(dev, pipe.rast.getNormalTextureView(), dst, cfg.width, cfg.height)
        assert got["sum_e"] == 0 and got["pixels"] == int((inner & (A >= 0.5)).sum()) > 0 and got["value"] == 0.0
    finally:
        dst.destroy()
        pipe.destroy()


# ---------------------------------------------------------------- 10. normalToRGBA8
@pytest.mark.parametrize("name", ["c1", "big-splats", "sparse"])
def test_normal_to_rgba8(hip_device, name):
    dev = hip_device
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    out = dev.createBuffer(4 * cfg.width * cfg.height)
    try:
        words, img = _normals(pipe)
        ops.normalToRGBA8(dev, pipe.rast.getNormalTextureView(), cfg.width, cfg.height, out)
        rgba = out.read(np.uint8).reshape(cfg.height, cfg.width, 4)
        want, v = n64.normal_to_rgba8_64(img)
        assert np.all(rgba[..., 3] == 255)
        none = np.linalg.norm(img[..., :3].astype(np.float64), axis=2) == 0
        assert np.all(rgba[..., :3][none] == 0) and (name != "sparse" or none.any())
        # per colour byte (a window of 2e-3 around each tie holds 0.2 % of uniformly spread values; per pixel that would be 0.6 %)
        ties = np.abs((v - np.floor(v)) - 0.5) < 1e-3
        diff = np.abs(rgba[..., :3].astype(np.int32) - want.astype(np.int32))
        print(f"normal_to_rgba8 {name}: ties {ties.mean():.4%} of the colour bytes, bytes off by one {np.mean(diff == 1):.4%}")
        assert ties.mean() <= MASK_CAP
        assert np.all(diff[~ties] == 0) and np.all(diff <= 1)
        assert rgba[..., 2][~none].mean() > 128, "the scenes' Gaussians face the camera: blue"
    finally:
        out.destroy()
        pipe.destroy()


# ---------------------------------------------------------------- 11. Viewer and Trainer
def test_viewer_render_normals_end_to_end(hip_device, tmp_path):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20_000, width=320, height=240)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8)[3]
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    v = Viewer(dev, cfg.width, cfg.height)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    out = dev.createBuffer(4 * cfg.width * cfg.height)
    try:
        v.setCamera(cam)
        v.setPointCloud(pc)                      # starts in point-cloud mode
        v.render(None)
        before = v.readFrame().copy()
        n = v.renderNormals()
        assert v._settings["renderMode"] == "pointcloud"
        assert n.dtype == np.float32 and n.shape == (cfg.height, cfg.width, 4)
        words, img = _normals(pipe)
        assert_bits_equal(n, img, "Viewer.renderNormals vs encodeNormal on a pipeline with the same camera")
        v.render(None)
        assert_bits_equal(v.readFrame(), before, "the frame after renderNormals")
        v.setRenderMode("gaussian")
        assert_bits_equal(v.renderNormals(), img, "renderNormals in gaussian mode")
        path = str(tmp_path / "normals.png")
        v.saveNormalPNG(path)
        with open(path, "rb") as f:
            png = images.decodePNG(f.read())
        ops.normalToRGBA8(dev, pipe.rast.getNormalTextureView(), cfg.width, cfg.height, out)
        assert_bits_equal(png, out.read(np.uint8).reshape(cfg.height, cfg.width, 4), "the PNG decodes to the kernel's bytes")
        assert png[..., 2].mean() > 128
    finally:
        out.destroy()
        pipe.destroy()
        v.destroy()


def test_trainer_normal_consistency_equals_the_ops_by_hand(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 6)
    t = _trainer(dev, cfg, g, sh, cameras[:4], imgs[:4], densify=False)
    dst = dev.createBuffer(16 * cfg.width * cfg.height)
    try:
        t.setEvaluationViews(cameras[4:], imgs[4:])
        for _ in range(6):
            t.step()
        ev = t.evaluate()
        r = t.normalConsistency()
        assert r["views"] == [0, 1] and r["iteration"] == ev["iteration"] and len(r["value"]) == 2
        ev2 = t.evaluate()
        assert ev2["sse"] == ev["sse"] and ev2["ssim"] == ev["ssim"], "evaluate()'s result is what it was"
        r_exp = t.normalConsistency([1], depthKind="expected")
        t.flushPointCloud()
        for kind, res, ids in (("median", r, [0, 1]), ("expected", r_exp, [1])):
            for slot, vid in enumerate(ids):
                cam = np.asarray(cameras[4 + vid]["camera"], np.float32)
                pipe_cam = dev.bufferFrom(cam)
                fw = ops.TiledForwardPass(dev, t.pointCloud, pipe_cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
                rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fw, format="rgba8unorm"))
                try:
                    fw.encode(None)
                    rast.encode(None, cfg.width, cfg.height)
                    rast.encodeDepth(None, (kind,))
                    rast.encodeNormal(None)
                    ops.depthToNormals(dev, rast.getDepthTextureView(kind), cfg.width, cfg.height, cam, dst)
                    hand = ops.normalAgreement(dev, rast.getNormalTextureView(), dst, cfg.width, cfg.height)
                finally:
                    rast.destroy()
                    fw.destroy()
                    pipe_cam.destroy()
                assert (res["sum_e"][slot], res["sum_a"][slot], res["pixels"][slot]) == (hand["sum_e"], hand["sum_a"], hand["pixels"]), (kind, vid)
                assert res["value"][slot] == hand["value"] and hand["pixels"] > 0
        assert r["mean"] == sum(r["sum_e"]) / sum(r["sum_a"])
        with pytest.raises(IndexError):
            t.normalConsistency([2])
        with pytest.raises(ValueError):
            t.normalConsistency(split="test")
        with pytest.raises(ValueError):
            t.normalConsistency(depthKind="weight_sum")
        t.step()
    finally:
        dst.destroy()
        t.destroy()
