"""GPU: TSDF fusion and mesh extraction (csrc/tsdf.hip).  integrate against the float64 restatement (tests/tsdf64.py) with a
derived bound outside its masks and both decisions inside them, the mesh against the restatement fed with the GPU's own volume (same triangles, same
order), the analytic sphere and a plane through voxel centres, determinism and recording, state and capacity errors, and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, loaders, ops, synth

import harness
import tsdf64 as t64
import test_tsdf_reference as R
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views
from test_tsdf_reference import MASK_CAP

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- helpers
def _read_volume(vol):
    nx, ny, nz = vol.dims
    T = vol.getTSDFBuffer().read(np.float32).reshape(nz, ny, nx).copy()
    W = vol.getWeightBuffer().read(np.float32).reshape(nz, ny, nx).copy()
    rgb = vol.getColourBuffer().read(np.float32).reshape(3, nz, ny, nx).copy() if vol.colour else None
    return T, W, rgb


def _write_volume(vol, T, W):
    vol.getTSDFBuffer().write(np.ascontiguousarray(T, np.float32))
    vol.getWeightBuffer().write(np.ascontiguousarray(W, np.float32))


def _sphere_inputs(dev):
    cams = R.sphere_cameras()
    out = []
    for c in cams:
        d, ws, col = R.sphere_depth(c)
        out.append(dict(camera=dev.bufferFrom(c), depth=dev.bufferFrom(d), ws=dev.bufferFrom(ws), colour=dev.bufferFrom(col)))
    return out


def _fuse_sphere(dev, dims, colour=True, views=range(6), inputs=None):
    inputs = inputs or _sphere_inputs(dev)
    vol = ops.TSDFVolume(dev, R.ORIGIN, R.VOXEL, dims, truncation=R.TRUNC, colour=colour)
    for v in views:
        i = inputs[v]
        vol.integrate(i["depth"], i["camera"], R.IMG_W, R.IMG_H, weightSum=i["ws"], colour=i["colour"] if colour else None)
    return vol


def _assert_volume_matches_float64(got, va, vb, reports, what):
    """The GPU's (T, W, rgb) against the restatement's two volumes (decisions on float32 values: A; on float64 values: B)."""
    T, W, rgb = got
    masks = R.union_masks(reports)
    share = {k: float(m.mean()) for k, m in masks.items()}
    assert all(s <= MASK_CAP for s in share.values()), f"{what}: {share}"
    masked = np.any(list(masks.values()), axis=0)
    bound = t64.tsdf_bound(max(r["scale"] for r in reports), max(r["max_depth"] for r in reports), va.truncation, len(reports))
    err_a, err_b = np.abs(T.astype(np.float64) - va.T), np.abs(T.astype(np.float64) - vb.T)
    print(f"tsdf accuracy {what}: max |T - T64| outside the masks = {err_a[~masked].max():.3e} = {err_a[~masked].max() / bound:.3f} of the bound {bound:.3e}; "
          f"masks {share}; updated voxels {(va.W > 0).mean():.1%}, max weight {va.W.max():.0f}")
    assert np.all(err_a[~masked] <= bound), f"{what}: T off by {err_a[~masked].max() / bound:.2f} x the bound"
    assert np.array_equal(W[~masked].astype(np.float64), va.W[~masked]), f"{what}: weights differ outside the masks"
    as_a = (err_a <= bound) & (W == va.W)
    as_b = (err_b <= bound) & (W == vb.W)
    assert np.all((as_a | as_b)[masked]), f"{what}: a masked voxel that follows neither decision"
    untouched = (va.W == 0) & (vb.W == 0)
    assert untouched.any()
    assert_bits_equal(T[untouched], np.ones(int(untouched.sum()), np.float32), f"{what}: untouched tsdf")
    assert_bits_equal(W[untouched], np.zeros(int(untouched.sum()), np.float32), f"{what}: untouched weight")
    if rgb is not None:
        assert np.all(rgb[:, untouched] == 0)
        err_c = np.abs(rgb.astype(np.float64) - va.rgb).max(axis=0)
        print(f"tsdf accuracy {what}: max colour error outside the masks = {err_c[~masked].max():.3e}")
        assert np.all(err_c[~masked] <= 1.0 / 255.0 + bound), f"{what}: colour"
    return masked


def _max_coordinate(origin, voxel, dims):
    o = np.asarray(origin, np.float64)
    return float(np.maximum(np.abs(o), np.abs(o + np.array(dims) * float(voxel))).max())


def _assert_mesh_matches_float64(vol, what, min_weight=1.0):
    """extractTriangles against mesh64 fed with the GPU's own float32 volume: no classification can tie."""
    T, W, rgb = _read_volume(vol)
    tri = vol.extractTriangles(min_weight)
    ref = t64.mesh64(T, W, vol.origin, vol.voxelSize, min_weight, rgb=rgb)
    assert tri["keys"].shape == ref["keys"].shape, f"{what}: {tri['keys'].shape[0]} triangles, the restatement has {ref['keys'].shape[0]}"
    assert np.array_equal(tri["keys"], ref["keys"]), f"{what}: key triples differ (triangles, their order or their winding)"
    tol = 4 * 2.0 ** -23 * _max_coordinate(vol.origin, vol.voxelSize, vol.dims)
    if tri["keys"].size:
        err = np.abs(tri["positions"].astype(np.float64) - ref["positions"]).max()
        print(f"mesh {what}: {tri['keys'].shape[0]} triangles, max position error {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}")
        assert err <= tol, f"{what}: positions off by {err / tol:.2f} x the bound"
        flat_k, flat_p = tri["keys"].reshape(-1), tri["positions"].reshape(-1, 3).view(np.uint32)
        order = np.argsort(flat_k, kind="stable")
        same = flat_k[order][1:] == flat_k[order][:-1]
        assert np.array_equal(flat_p[order][1:][same], flat_p[order][:-1][same]), f"{what}: equal keys with different position bits"
        if rgb is not None:
            assert np.all(tri["colours"][..., 3] == 255)
            # the byte is rint of 255 x a value within a few float32 roundings of the float64 one
            cerr = np.abs(tri["colours"][..., :3].astype(np.float64) - 255.0 * np.clip(ref["colours"], 0, 1)).max()
            assert cerr <= 0.5 + 1e-3, f"{what}: vertex colours off by {cerr}"
    return tri, ref


# ---------------------------------------------------------------- 1. integrate against the restatement
@pytest.mark.parametrize("dims", [R.SPHERE_DIMS, (33, 17, 9)])
def test_integrate_sphere_matches_float64(hip_device, dims):
    vol = _fuse_sphere(hip_device, dims)
    try:
        va, vb, reports = R.fuse_sphere64(dims)
        _assert_volume_matches_float64(_read_volume(vol), va, vb, reports, f"sphere {dims}")
        _assert_mesh_matches_float64(vol, f"fused sphere {dims}")
    finally:
        vol.destroy()


SCENE_DIMS = (96, 96, 96)
SCENE_VOXEL = 8.0 / 96.0
SCENE_ORIGIN = (-4.013, -3.987, 2.009)    # the scene's box: z in [2, 10], x and y the frustum's width there; off the round numbers


def _scene_cfg():
    return harness.small_config("c2", num_points=20_000, width=320, height=240)


def _scene_views(dev, cfg, n_views=4):
    """The 20 000-point scene from ``n_views`` circle cameras: per view the camera block and host copies of depth, weight sum and colour, and the device
    buffers they were read from (kept alive by the pipeline, which is returned too)."""
    g, sh = synth.make_gaussians(cfg)
    cams = synth.circle_cameras(cfg, n_views)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cams[0])
    views = []
    for c in cams:
        pipe.camera.write(c)
        pipe.forward()
        pipe.rast.encodeDepth(None, ("median", "weight_sum"))
        dev.synchronize()
        n = cfg.width * cfg.height
        views.append(dict(camera=c, depth=pipe.rast.getDepthTextureView("median").read(np.float32, count=n), ws=pipe.rast.getDepthTextureView("weight_sum").read(np.float32, count=n),
                          colour=pipe.rast.getOutputTextureView().read(np.uint8, count=4 * n).reshape(-1, 4)))
    return pipe, views


def _fuse_scene(dev, cfg, views, colour=True):
    vol = ops.TSDFVolume(dev, SCENE_ORIGIN, SCENE_VOXEL, SCENE_DIMS, colour=colour)
    for v in views:
        cam, d, ws, col = dev.bufferFrom(v["camera"]), dev.bufferFrom(v["depth"]), dev.bufferFrom(v["ws"]), dev.bufferFrom(v["colour"])
        vol.integrate(d, cam, cfg.width, cfg.height, weightSum=ws, colour=col if colour else None)
    dev.synchronize()
    return vol


def test_integrate_scene_matches_float64(hip_device):
    """96^3 voxels fused from four 320 x 240 median-depth images of the 20 000-point scene."""
    dev, cfg = hip_device, _scene_cfg()
    pipe, views = _scene_views(dev, cfg)
    vol = None
    try:
        vol = _fuse_scene(dev, cfg, views)
        assert abs(vol.truncation - 4 * SCENE_VOXEL) < 1e-6
        va = t64.Volume64(SCENE_ORIGIN, SCENE_VOXEL, SCENE_DIMS, vol.truncation)
        vb = va.copy()
        reports = [t64.integrate64(va, vb, v["depth"], v["camera"], cfg.width, cfg.height, weight_sum=v["ws"], colour=v["colour"]) for v in views]
        assert 8 * max(r["dist_px"] for r in reports) <= t64.EPS_PIXEL and 8 * max(r["dist_sdf"] for r in reports) <= t64.EPS_SDF
        print(f"scene: largest |f32 - f64| px / W, py / H {max(r['dist_px'] for r in reports):.3e}, sdf / truncation {max(r['dist_sdf'] for r in reports):.3e}")
        _assert_volume_matches_float64(_read_volume(vol), va, vb, reports, "scene 96^3")
        assert (va.W > 0).mean() > 0.01 and va.W.max() == 4
        total = vol.countTriangles()
        assert total > 0
    finally:
        if vol is not None:
            vol.destroy()
        pipe.destroy()


# ---------------------------------------------------------------- 2. the mesh
@pytest.mark.parametrize("dims,shift", [(R.SPHERE_DIMS, (0.07, -0.11, 0.05)), ((33, 17, 9), (0.9, -0.6, -0.45)), ((70, 5, 3), None)])
def test_analytic_sphere_mesh(hip_device, dims, shift):
    """A volume written directly with the analytic field of a sphere: a closed, outward, genus-0 mesh near the sphere, triangle for triangle the
    restatement's.  (70 x 5 x 3: more than one wave along x; the sphere leaves that volume, so only the comparison is made there.)"""
    dev = hip_device
    vol = ops.TSDFVolume(dev, R.ORIGIN, R.VOXEL, dims, truncation=R.TRUNC, colour=False)
    try:
        radius = R.RADIUS if dims == R.SPHERE_DIMS else 2.9 * R.VOXEL
        centre = (R.ORIGIN.astype(np.float64) + 0.5 * np.array(dims) * R.VOXEL) + np.array(shift or (0.3, 0.2, 0.1)) * R.VOXEL
        x, y, z = t64._grid(t64.Volume64(R.ORIGIN, R.VOXEL, dims, R.TRUNC).centres64())
        T = np.clip((np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius) / R.TRUNC, -1, 1).astype(np.float32)
        _write_volume(vol, T, np.ones(T.shape, np.float32))
        tri, _ = _assert_mesh_matches_float64(vol, f"analytic sphere {dims}")
        if shift is not None:
            topo = R.assert_closed_sphere_mesh(tri["keys"], tri["positions"], centre, radius, f"GPU mesh {dims}")
            mesh = vol.extractMesh()
            assert mesh["vertices"].shape == (topo["V"], 3) and mesh["faces"].shape == (topo["F"], 3) and mesh["colours"] is None
            assert np.all(np.diff(mesh["keys"].astype(np.int64)) > 0)
            assert_bits_equal(mesh["vertices"][mesh["faces"]], tri["positions"], "welded vertices give back the emitted positions")
    finally:
        vol.destroy()


def test_plane_through_voxel_centres(hip_device):
    """T == 0 on a layer: 0 is outside, the surface runs through that layer's voxel centres, zero-area triangles are emitted and nothing faults; a voxel
    of weight below min_weight takes its cells out."""
    vol = ops.TSDFVolume(hip_device, (0, 0, 0), 1.0, (4, 5, 6), truncation=2.0, colour=False)
    try:
        T = np.ones((6, 5, 4), np.float32)
        T[:2] = -1.0
        T[2] = 0.0
        W = np.full(T.shape, 2.0, np.float32)
        _write_volume(vol, T, W)
        tri, ref = _assert_mesh_matches_float64(vol, "plane", min_weight=2.0)
        assert tri["keys"].shape[0] == ref["keys"].shape[0] > 0 and np.all(tri["positions"][..., 2] == 2.5)
        area = np.linalg.norm(np.cross(tri["positions"][:, 1] - tri["positions"][:, 0], tri["positions"][:, 2] - tri["positions"][:, 0]), axis=1)
        assert (area == 0).any() and np.isclose(area.sum() / 2.0, 12.0)
        W[2, 2, 2] = 1.0
        _write_volume(vol, T, W)
        tri2, _ = _assert_mesh_matches_float64(vol, "plane with a hole", min_weight=2.0)
        assert tri2["keys"].shape[0] < tri["keys"].shape[0]
        assert vol.countTriangles(1.0) == tri["keys"].shape[0]
    finally:
        vol.destroy()


# ---------------------------------------------------------------- 3. determinism and recording
def test_fusion_and_extraction_are_deterministic_and_record(hip_device):
    dev = hip_device
    inputs = _sphere_inputs(dev)
    a = _fuse_sphere(dev, (33, 17, 9), inputs=inputs)
    b = _fuse_sphere(dev, (33, 17, 9), inputs=inputs)
    c = ops.TSDFVolume(dev, R.ORIGIN, R.VOXEL, (33, 17, 9), truncation=R.TRUNC)
    try:
        va, vb_ = _read_volume(a), _read_volume(b)
        for x, y, k in zip(va, vb_, ("tsdf", "weight", "rgb")):
            assert_bits_equal(x, y, f"two fusions: {k}")
        ta, tb = a.extractTriangles(), b.extractTriangles()
        for k in ("positions", "keys", "colours"):
            assert_bits_equal(ta[k], tb[k], f"two extractions: {k}")
        assert ta["keys"].shape[0] > 0
        # integrate recorded into a command buffer and replayed equals the eager calls
        with dev.createCommandEncoder("fuse", record=True) as enc:
            for i in inputs:
                c.integrate(i["depth"], i["camera"], R.IMG_W, R.IMG_H, weightSum=i["ws"], colour=i["colour"])
            cmd = enc.finish()
        assert np.all(_read_volume(c)[1] == 0), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        for x, y, k in zip(_read_volume(c), va, ("tsdf", "weight", "rgb")):
            assert_bits_equal(x, y, f"recorded integrate: {k}")
        with pytest.raises(_lib.StateError):      # the count waits for its total
            with dev.createCommandEncoder("doomed", record=True) as enc:
                c.countTriangles()
        dev.synchronize()
        cmd.destroy()
        # reset gives back the fresh state
        a.reset()
        T, W, rgb = _read_volume(a)
        assert np.all(T == 1) and np.all(W == 0) and np.all(rgb == 0)
        assert a.countTriangles() == 0
    finally:
        for v in (a, b, c):
            v.destroy()


# ---------------------------------------------------------------- 4. state and capacity
def test_state_capacity_and_argument_errors(hip_device):
    dev = hip_device
    lib = dev.lib
    inputs = _sphere_inputs(dev)
    vol = _fuse_sphere(dev, R.SPHERE_DIMS, views=[0, 3], inputs=inputs)
    plain = ops.TSDFVolume(dev, R.ORIGIN, R.VOXEL, (5, 4, 3), colour=False)
    try:
        i0 = inputs[0]
        out = dev.createBuffer(36 * 20000)
        keys = dev.createBuffer(24 * 20000)
        with pytest.raises(_lib.StateError):      # emit before any count
            _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, keys.ptr, None, 20000))
        total = vol.countTriangles()
        assert 0 < total <= 20000
        vol.integrate(i0["depth"], i0["camera"], R.IMG_W, R.IMG_H)
        with pytest.raises(_lib.StateError):      # the volume was integrated since the count
            _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, keys.ptr, None, 20000))
        total = vol.countTriangles()
        vol.reset()
        with pytest.raises(_lib.StateError):      # ... or reset
            _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, keys.ptr, None, 20000))
        for v in (0, 3):
            vol.integrate(inputs[v]["depth"], inputs[v]["camera"], R.IMG_W, R.IMG_H, weightSum=inputs[v]["ws"], colour=inputs[v]["colour"])
        total = vol.countTriangles()
        vol.getWeightBuffer()
        with pytest.raises(_lib.StateError):      # ... or handed out for writing
            _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, keys.ptr, None, 20000))
        total = vol.countTriangles()
        marker = np.full(9 * 20000, 0x7FC01234, np.uint32)
        out.write(marker)
        with pytest.raises(_lib.CapacityError):
            _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, keys.ptr, None, total - 1))
        dev.synchronize()
        assert_bits_equal(out.read(np.uint32), marker, "a refused emit writes nothing")
        _lib.check(lib.wdgs_tsdf_volume_emit_triangles(vol.handle, out.ptr, None, None, total))     # keys and colours are optional
        got = out.read(np.uint32)
        assert np.all(got[9 * total:] == 0x7FC01234) and not np.any(got[:9 * total] == 0x7FC01234)
        # a wrong image size, colour to a colourless volume
        with pytest.raises(_lib.StateError):
            vol.integrate(i0["depth"], i0["camera"], R.IMG_H, R.IMG_W)
        with pytest.raises(_lib.StateError):
            plain.integrate(i0["depth"], i0["camera"], R.IMG_W, R.IMG_H, colour=i0["colour"])
        with pytest.raises(_lib.StateError):
            plain.getColourBuffer()
        before = _read_volume(vol)
        with dev.createCommandEncoder("wrong size", record=True) as enc:     # recorded, the size cannot be checked on the host: the kernel writes nothing
            vol.integrate(i0["depth"], i0["camera"], R.IMG_H, R.IMG_W)
            cmd = enc.finish()
        dev.queue.submit([cmd])
        dev.synchronize()
        cmd.destroy()
        for x, y in zip(_read_volume(vol), before):
            assert_bits_equal(x, y, "a recorded integrate with the wrong image size")
        # an empty volume
        assert plain.countTriangles() == 0
        tri = plain.extractTriangles()
        assert tri["positions"].shape == (0, 3, 3) and tri["keys"].shape == (0, 3) and tri["colours"] is None
        mesh = plain.extractMesh()
        assert mesh["vertices"].shape == (0, 3) and mesh["faces"].shape == (0, 3) and mesh["keys"].shape == (0,)
        # create's arguments
        for kw in (dict(dims=(1, 4, 4)), dict(dims=(4, 4, 1)), dict(dims=(1024, 1024, 257)), dict(dims=(65536, 65536, 2)), dict(voxelSize=0.0), dict(voxelSize=float("inf")),
                   dict(voxelSize=-1.0), dict(truncation=0.0), dict(truncation=float("nan")), dict(maxWeight=0.0)):
            args = dict(origin=(0, 0, 0), voxelSize=0.1, dims=(4, 4, 4))
            args.update(kw)
            with pytest.raises(_lib.WdgsError) as e:
                ops.TSDFVolume(dev, **args)
            assert e.value.code == _lib.WDGS_E_INVALID, kw
        with pytest.raises(_lib.WdgsError) as e:
            plain.countTriangles(0.0)
        assert e.value.code == _lib.WDGS_E_INVALID
        v = ops.TSDFVolume.fromBounds(dev, (0, 0, 0), (1.0, 0.55, 0.31), 0.1, colour=False)
        assert v.dims == (10, 6, 4) and abs(v.truncation - 0.4) < 1e-6
        v.destroy()
        out.destroy()
        keys.destroy()
    finally:
        vol.destroy()
        plain.destroy()
        plain.destroy()   # idempotent


# ---------------------------------------------------------------- 5. the Trainer surface
def test_trainer_fuse_depth_and_extract_mesh(hip_device, tmp_path):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    hand = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    try:
        for _ in range(4):
            t.step()
        t.drain()
        frame = t.rasterizer.getOutputTextureView().read(np.uint32).copy()
        iteration, rng_state = t.iteration, t._rng.getstate()
        assert t.fuseDepth(vol, [2, 0]) == [2, 0]
        assert t.iteration == iteration and t._rng.getstate() == rng_state
        assert_bits_equal(t.rasterizer.getOutputTextureView().read(np.uint32), frame, "the training rasterizer's output frame")
        t.flushPointCloud()
        for vid in (2, 0):
            cam = dev.bufferFrom(np.asarray(cameras[vid]["camera"], np.float32))
            fw = ops.TiledForwardPass(dev, t.pointCloud, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
            rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fw, format="rgba8unorm"))
            try:
                fw.encode(None)
                rast.encode(None, cfg.width, cfg.height)
                rast.encodeDepth(None, ("median", "weight_sum"))
                hand.integrate(rast.getDepthTextureView("median"), cam, cfg.width, cfg.height, weightSum=rast.getDepthTextureView("weight_sum"),
                               colour=rast.getOutputTextureView())
                dev.synchronize()
            finally:
                rast.destroy()
                fw.destroy()
        got, want = _read_volume(vol), _read_volume(hand)
        assert (want[1] > 0).any() and (want[0] < 0).any()
        for x, y, k in zip(got, want, ("tsdf", "weight", "rgb")):
            assert_bits_equal(x, y, f"fuseDepth vs the ops by hand: {k}")
        mesh = t.extractMesh(lo, hi, voxel)
        assert t.iteration == iteration and t._rng.getstate() == rng_state
        assert mesh["faces"].shape[0] > 0 and mesh["vertices"].shape[0] > 0 and mesh["colours"].shape == mesh["vertices"].shape
        assert int(mesh["faces"].max()) == mesh["vertices"].shape[0] - 1
        top = np.asarray(lo) + np.array(vol.dims) * voxel
        assert np.all(mesh["vertices"] >= np.asarray(lo, np.float32)) and np.all(mesh["vertices"] <= top.astype(np.float32))
        path = str(tmp_path / "scene.ply")
        loaders.saveMeshPLY(path, mesh)
        back = loaders.loadMeshPLY(path)
        assert_bits_equal(back["vertices"], mesh["vertices"], "PLY vertices")
        assert_bits_equal(back["faces"], mesh["faces"], "PLY faces")
        assert_bits_equal(back["colours"], mesh["colours"], "PLY colours")
        with pytest.raises(ValueError):
            t.fuseDepth(vol, depthKind="weight_sum")
        with pytest.raises(IndexError):
            t.fuseDepth(vol, [4])
        t.step()
        assert t.iteration == iteration + 1
    finally:
        vol.destroy()
        hand.destroy()
        t.destroy()
