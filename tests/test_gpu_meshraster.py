"""GPU: the mesh rasterizer and the depth agreement on the device (csrc/meshraster.hip).  Every byte of every output equals the
restatement (tests/meshraster_ref.py) on its crafted cases -- empty inputs, pixel centres on shared edges and vertices, equal depths, every face class, bounding
boxes either side of the threshold between the two kernels, both kernels into one image, more work items than the block kernel's grid has waves, the icosphere
under rolled, steep and close cameras, the cull modes -- then the subsets of the outputs, argument and state errors, recording, repeats and reuse, the
two-sphere TSDF volume, and the Trainer and Viewer surfaces."""
import itertools

import numpy as np
import pytest

from webdgs_amd import _lib, ops, synth
from webdgs_amd.viewer import Viewer

import harness
import meshclean_ref as M
import meshraster_ref as R
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
BYTES = dict(depth=4, face=4, colour=4, normal=16)
SHAPES = dict(depth=lambda h, w: (h, w), face=lambda h, w: (h, w), colour=lambda h, w: (h, w, 4), normal=lambda h, w: (h, w, 4))


def _upload(dev, m):
    return dict(vertices=dev.bufferFrom(m["vertices"]), faces=dev.bufferFrom(m["faces"]), colours=None if m["colours"] is None else dev.bufferFrom(m["colours"]),
                camera=dev.bufferFrom(m["camera"]), V=m["vertices"].shape[0], F=m["faces"].shape[0])


def _images(dev, w, h, names, fill=None):
    out = {k: dev.createBuffer(BYTES[k] * w * h, f"mesh {k}") for k in names}
    if fill is not None:
        for b in out.values():
            b.write(np.full(b.size // 4, fill, np.uint32))
    return out


def _read(outs, w, h):
    return {k: b.read(ops.RASTER_OUTPUTS[k][1], count=int(np.prod(SHAPES[k](h, w)))).reshape(SHAPES[k](h, w)) for k, b in outs.items()}


def _run(dev, rasterizer, m, names=None):
    """Everything one ``MeshRasterizer`` gives for case ``m``: the images of ``names`` (default: all the case can have) and ``stats``."""
    names = [k for k in R.OUTPUTS if k != "colour" or m["colours"] is not None] if names is None else names
    src = _upload(dev, m)
    w, h = m["width"], m["height"]
    outs = _images(dev, w, h, names, SENTINEL)
    rasterizer.encode(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], src["camera"], w, h, m["near"], m["cull"], **outs)
    got = dict(_read(outs, w, h), stats=rasterizer.stats())
    dev.synchronize()
    for b in list(outs.values()) + [src[k] for k in ("vertices", "faces", "colours", "camera") if src[k] is not None]:
        b.destroy()
    return got


def _assert_result(got, want, what, names=None):
    for k in (R.OUTPUTS if names is None else names):
        if want.get(k) is None:
            assert k not in got, f"{what}: {k}"
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")
    assert got["stats"] == want["stats"], f"{what}: {got['stats']}"


# ---------------------------------------------------------------- 1. the crafted cases
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_device_images_equal_the_restatement(hip_device, name):
    dev = hip_device
    m, want = R.case(name), R.expected(name)
    rasterizer = ops.MeshRasterizer(dev)
    try:
        got = _run(dev, rasterizer, m)
    finally:
        rasterizer.destroy()
    _assert_result(got, want, name)
    for k, n in R.EXPECT.get(name, {}).items():
        assert got["stats"][k] == n, f"{name}: {k}"
    assert R.digest(got) == R.digest(want)
    # the one-call form
    names = tuple(k for k in R.OUTPUTS if want.get(k) is not None)
    one = ops.rasterizeMesh(dev, dict(vertices=m["vertices"], faces=m["faces"], colours=m["colours"]), m["camera"], m["width"], m["height"], m["near"], m["cull"], names)
    _assert_result(one, want, f"rasterizeMesh: {name}")


def test_cull_back_leaves_the_closed_sphere_unchanged_and_front_does_not(hip_device):
    dev = hip_device
    m = R.case("sphere-roll37")
    mesh = dict(vertices=m["vertices"], faces=m["faces"])
    none, back, front = (ops.rasterizeMesh(dev, mesh, m["camera"], m["width"], m["height"], cull=c, outputs=("depth",)) for c in ("none", "back", "front"))
    assert_bits_equal(back["depth"], none["depth"], "cull='back' on a closed sphere seen from outside")
    assert not np.array_equal(front["depth"].view(np.uint32), none["depth"].view(np.uint32))
    assert back["stats"]["culledFaces"] > 0 and front["stats"]["culledFaces"] == 320 - back["stats"]["culledFaces"]


@pytest.mark.parametrize("name", ["mixed-67x45", "classes"])
def test_every_subset_of_the_outputs(hip_device, name):
    dev = hip_device
    m, want = R.case(name), R.expected(name)
    rasterizer = ops.MeshRasterizer(dev)
    try:
        for r in range(0, 5):
            for names in itertools.combinations(R.OUTPUTS, r):
                got = _run(dev, rasterizer, m, list(names))
                assert sorted(got) == sorted(list(names) + ["stats"])
                _assert_result(got, want, f"{name}: outputs {names}", names)
    finally:
        rasterizer.destroy()


# ---------------------------------------------------------------- 2. errors, recording, repeats
def test_arguments_state_and_recording(hip_device):
    dev = hip_device
    m, want = R.case("mixed-67x45"), R.expected("mixed-67x45")
    src = _upload(dev, m)
    V, F, w, h = src["V"], src["F"], m["width"], m["height"]
    outs = _images(dev, w, h, R.OUTPUTS, SENTINEL)
    rasterizer = ops.MeshRasterizer(dev)
    encode = lambda **kw: rasterizer.encode(**dict(dict(vertices=src["vertices"], numVertices=V, faces=src["faces"], numFaces=F, colours=src["colours"],
                                                        camera=src["camera"], width=w, height=h, near=m["near"], cull="none"), **dict(outs, **kw)))
    try:
        with pytest.raises(_lib.StateError):   # no encode precedes it
            rasterizer.stats()
        bad = (dict(numVertices=2 ** 31), dict(numFaces=2 ** 32 // 3 + 1), dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(near=0.0),
               dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(cull="sideways"), dict(colours=None), dict(vertices=None), dict(faces=None))
        for kw in bad:
            with pytest.raises(_lib.WdgsError) as e:
                encode(**kw)
            assert e.value.code == _lib.WDGS_E_INVALID, kw
        for k in ("vertices", "faces", "colours", "camera", "depth", "face", "colour", "normal"):   # a misaligned pointer
            b = dict(src, **outs)[k]
            with pytest.raises(_lib.WdgsError) as e:
                encode(**{k: dev.view(b.ptr + 2, b.size)})   # (refused before anything is read: the view's size is never used)
            assert e.value.code == _lib.WDGS_E_INVALID, k
        with pytest.raises(_lib.WdgsError) as e:   # the normal image: 16 bytes
            encode(normal=dev.view(outs["normal"].ptr + 4, outs["normal"].size))
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.StateError):   # still no encode
            rasterizer.stats()
        with pytest.raises(_lib.StateError):   # a call that has to grow the object's arrays cannot be recorded
            with dev.createCommandEncoder("doomed", record=True):
                encode()
        dev.synchronize()
        for k, b in outs.items():
            assert np.all(b.read(np.uint32) == SENTINEL), f"a refused call wrote {k}"
        encode()
        eager = dict(_read(outs, w, h), stats=rasterizer.stats())
        _assert_result(eager, want, "after the refusals")
        # an encode that grows nothing waits for nothing and records
        for b in outs.values():
            b.clear()
        with dev.createCommandEncoder("mesh raster", record=True) as enc:
            encode()
            with pytest.raises(_lib.StateError):   # the statistics wait
                rasterizer.stats()
            cmd = enc.finish()
        assert all(not b.read(np.uint32).any() for b in outs.values()), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        _assert_result(dict(_read(outs, w, h), stats=rasterizer.stats()), eager, "recorded and replayed")
        dev.queue.submit([cmd])
        dev.synchronize()
        _assert_result(dict(_read(outs, w, h), stats=rasterizer.stats()), eager, "replayed again")
        cmd.destroy()
        with pytest.raises(ValueError):
            encode(depth=dev.view(outs["depth"].ptr, outs["depth"].size - 4))
        with pytest.raises(ValueError):
            ops.rasterizeMesh(dev, dict(vertices=m["vertices"], faces=m["faces"]), m["camera"], w, h, outputs=("depth", "albedo"))
        with pytest.raises(_lib.WdgsError):   # a colour image of a mesh without colours
            ops.rasterizeMesh(dev, dict(vertices=m["vertices"], faces=m["faces"], colours=None), m["camera"], w, h, outputs=("colour",))
    finally:
        rasterizer.destroy()
        rasterizer.destroy()   # idempotent
        for b in list(outs.values()) + [src[k] for k in ("vertices", "faces", "colours", "camera")]:
            b.destroy()


def test_two_runs_agree_and_one_object_takes_meshes_and_viewports_of_any_size(hip_device):
    dev = hip_device
    m = R.case("mixed-67x45")
    mesh = dict(vertices=m["vertices"], faces=m["faces"], colours=m["colours"])
    a, b = (ops.rasterizeMesh(dev, mesh, m["camera"], m["width"], m["height"], outputs=R.OUTPUTS) for _ in range(2))
    for k in R.OUTPUTS:
        assert_bits_equal(b[k], a[k], f"a second run: {k}")
    assert a["stats"] == b["stats"]
    rasterizer = ops.MeshRasterizer(dev)
    try:
        for name in ("triangle-on-centres", "forty-layers", "one-pixel", "mixed-67x45", "nothing", "sphere-close", "no-faces", "fan-65", "classes", "no-vertices",
                     "forty-layers", "threshold-above-x"):
            _assert_result(_run(dev, rasterizer, R.case(name)), R.expected(name), f"reused object: {name}")
    finally:
        rasterizer.destroy()


def test_one_encode_launch_for_launch(hip_device):
    """The launch sequence of one encode, pinned: each of the four kernels once and the library's scan once."""
    dev = hip_device
    m = R.case("mixed-67x45")
    src = _upload(dev, m)
    outs = _images(dev, m["width"], m["height"], R.OUTPUTS)
    rasterizer = ops.MeshRasterizer(dev)
    try:
        dev.synchronize()
        dev.setProfiling(True)
        dev.kernelTimes(reset=True)
        rasterizer.encode(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], src["camera"], m["width"], m["height"], **outs)
        dev.synchronize()
        dev.setProfiling(False)
        times = dev.kernelTimes(reset=True)
    finally:
        dev.setProfiling(False)
        rasterizer.destroy()
    launches = {k: v[0] for k, v in times.items()}
    print("launches:", sorted(launches.items()))
    assert {k: n for k, n in launches.items() if k.startswith("raster_")} == dict(raster_vertices=1, raster_faces=1, raster_blocks=1, raster_resolve=1), launches
    assert {k: n for k, n in launches.items() if k.startswith("scan_")} == dict(scan_reduce=1, scan_block_sums=1, scan_downsweep=1), launches


# ---------------------------------------------------------------- 3. depth agreement
@pytest.mark.parametrize("name", sorted(R.AGREEMENT_CASES))
def test_depth_agreement_equals_the_restatement(hip_device, name):
    dev = hip_device
    c, want = R.AGREEMENT_CASES[name], R.agreement_expected(name)
    got = ops.depthAgreement(dev, c["a"], c["b"], c["width"], c["height"], c["max_difference"], c["threshold"], c["weight_sum"], c["min_weight_sum"])
    assert [got[k] for k in ("both", "onlyA", "onlyB", "within", "sum_q")] == want, name
    if want[0]:
        assert got["mean"] == want[4] * float(np.float32(c["max_difference"])) / 2.0 ** 24 / want[0]
    else:
        assert np.isnan(got["mean"])
    if name in R.AGREEMENT_EXPECT:
        assert want == R.AGREEMENT_EXPECT[name]


def test_depth_agreement_arguments_and_recording(hip_device):
    dev = hip_device
    c, want = R.AGREEMENT_CASES["random-67x45"], R.agreement_expected("random-67x45")
    a, b, ws = dev.bufferFrom(c["a"]), dev.bufferFrom(c["b"]), dev.bufferFrom(c["weight_sum"])
    out = dev.createBuffer(48)
    out.write(np.full(12, SENTINEL, np.uint32))
    w, h = c["width"], c["height"]
    try:
        for md, th in ((0.0, 0.1), (1.0, 0.0), (0.1, 0.2), (float("nan"), 0.1), (1.0, float("inf")), (float("inf"), 1.0), (-1.0, -2.0)):
            with pytest.raises(_lib.WdgsError) as e:
                ops.encodeDepthAgreement(dev, a, b, w, h, md, th, out)
            assert e.value.code == _lib.WDGS_E_INVALID, (md, th)
        with pytest.raises(_lib.WdgsError):
            ops.encodeDepthAgreement(dev, a, b, w, h, 1.0, 0.5, dev.view(out.ptr + 4, 40))   # the sums are 8-byte aligned
        dev.synchronize()
        assert np.all(out.read(np.uint32) == SENTINEL), "a refused call wrote the sums"
        with dev.createCommandEncoder("depth agreement", record=True) as enc:
            ops.encodeDepthAgreement(dev, a, b, w, h, c["max_difference"], c["threshold"], out, ws, c["min_weight_sum"])
            cmd = enc.finish()
        assert np.all(out.read(np.uint32) == SENTINEL), "recording runs nothing"
        for _ in range(2):   # the sums are cleared by the call itself
            dev.queue.submit([cmd])
            dev.synchronize()
            assert [int(x) for x in out.read(np.uint64, count=5)] == want
        assert np.all(out.read(np.uint32, offset=40) == SENTINEL)
        cmd.destroy()
    finally:
        for x in (a, b, ws, out):
            x.destroy()


# ---------------------------------------------------------------- 4. two spheres in a TSDF volume
def _two_sphere_depth(cam, w, h, shift):
    """The depth image f32[h, w] of the two spheres of meshclean_ref, moved by ``shift`` in view space, under an identity-rotation camera: float64 ray-sphere
    intersections at the pixel centres, 0 where the ray misses both."""
    j, i = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    d = np.stack([(2.0 * i / w - 1.0) / float(cam[32]), (2.0 * j / h - 1.0) / float(-cam[37]), np.ones_like(i)], axis=-1)
    depth = np.full((h, w), np.inf)
    for s in (M.TS_A, M.TS_B):
        c = s["centre"] + shift
        a, b, cc = np.sum(d * d, axis=-1), -2.0 * d @ c, float(c @ c) - s["radius"] ** 2
        disc = b * b - 4.0 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
        depth = np.minimum(depth, t)
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)


def test_a_fused_view_agrees_with_its_mesh_better_than_with_the_mesh_moved_two_voxels(hip_device):
    dev = hip_device
    w, h, fy = 160, 96, 200.0
    shift = np.array([0.0, 0.0, 3.0])
    view = np.eye(4)
    view[:3, 3] = shift
    cam = synth.camera_block(view, w, h, fy)
    depth = _two_sphere_depth(cam, w, h, shift)
    assert (depth > 0).sum() > 1000
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=False)
    depth_buf, cam_buf = dev.bufferFrom(depth), dev.bufferFrom(cam)
    welded = {}
    try:
        vol.integrate(depth_buf, cam_buf, w, h)
        mesh = vol.extractMesh()
        assert mesh["faces"].shape[0] > 1000
        moved = dict(mesh, vertices=(mesh["vertices"] + np.array([0.0, 0.0, 2.0 * M.TS_VOXEL], np.float32)).astype(np.float32))
        here, there = (ops.rasterizeMesh(dev, x, cam, w, h, outputs=("depth", "face")) for x in (mesh, moved))
        want = R.rasterize(mesh["vertices"], mesh["faces"], None, cam, w, h, ops.MESH_RASTER_NEAR)
        _assert_result(here, want, "the fused view's mesh", ("depth", "face"))
        near, far = (ops.depthAgreement(dev, x["depth"], depth, w, h, maxDifference=0.5, threshold=M.TS_VOXEL) for x in (here, there))
        print(f"fused view against its mesh: {near}; against the mesh moved two voxels: {far}")
        assert near["both"] > 1000 and far["both"] > 1000
        assert near["mean"] < far["mean"]
        # the welded mesh as buffers, where the volume emitted it
        tri = vol.extractTriangleBuffers()
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        ops.destroyBuffers(tri)
        bufs = ops.rasterizeMesh(dev, welded, cam_buf, w, h, outputs=("depth", "face", "normal"), asBuffers=True)
        try:
            got = dict(_read({k: bufs[k] for k in ("depth", "face", "normal")}, w, h), stats=bufs["stats"])
        finally:
            ops.destroyBuffers({k: bufs[k] for k in ("depth", "face", "normal")})
        _assert_result(got, want, "weld='device' buffers", ("depth", "face", "normal"))
        assert_bits_equal(welded["vertices"].read(np.float32).reshape(-1, 3), mesh["vertices"], "the input is left as it is")
    finally:
        ops.destroyBuffers(welded)
        depth_buf.destroy()
        cam_buf.destroy()
        vol.destroy()


# ---------------------------------------------------------------- 5. the Trainer and Viewer surfaces
def _state_digest(t):
    import hashlib
    t.flushPointCloud()
    hsh = hashlib.sha256()
    hsh.update(t.pointCloud.gaussian_3d_buffer.read(np.uint32).tobytes())
    hsh.update(t.pointCloud.sh_buffer.read(np.uint32).tobytes())
    return hsh.hexdigest(), t.iteration, t._rng.getstate()


def test_trainer_mesh_depth_agreement_leaves_training_alone(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    try:
        for _ in range(4):
            t.step()
        t.drain()
        mesh = t.extractMesh(lo, hi, voxel)
        assert mesh["faces"].shape[0] > 0
        before = _state_digest(t)
        out = t.meshDepthAgreement(mesh, split="train", maxDifference=1.0, threshold=voxel)
        assert out["views"] == [0, 1, 2, 3] and out["iteration"] == t.iteration
        for i in range(4):
            assert out["both"][i] + out["onlyA"][i] + out["onlyB"][i] <= cfg.width * cfg.height
            assert out["within"][i] <= out["both"][i] and out["both"][i] > 0 and np.isfinite(out["mean"][i])
        assert out["total"]["both"] == sum(out["both"]) and np.isfinite(out["total"]["mean"])
        one = t.meshDepthAgreement(mesh, viewIds=[2], split="train", maxDifference=1.0, threshold=voxel)
        assert [one[k][0] for k in ("both", "onlyA", "onlyB", "within", "sum_q")] == [out[k][2] for k in ("both", "onlyA", "onlyB", "within", "sum_q")]
        assert _state_digest(t) == before
    finally:
        t.destroy()


def test_viewer_renders_a_mesh_in_its_four_modes(hip_device, tmp_path):
    dev = hip_device
    m = R.case("sphere-roll37")
    mesh = dict(vertices=m["vertices"], faces=m["faces"], colours=m["colours"])
    w, h = m["width"], m["height"]
    viewer = Viewer(dev, w, h)
    try:
        viewer.setCamera(m["camera"])
        want = R.expected("sphere-roll37")
        hit = want["face"] != R.NO_FACE
        images = {mode: viewer.renderMesh(mesh, mode) for mode in ("colour", "depth", "normal", "face")}
        for mode, img in images.items():
            assert img.shape == (h, w, 4) and img.dtype == np.uint8, mode
        assert_bits_equal(images["colour"], want["colour"], "renderMesh: colour")
        assert np.array_equal(np.all(images["face"] == 0, axis=-1), ~hit), "face mode is black exactly where the face image is empty"
        assert np.array_equal(images["face"], ops.faceIndexColours(want["face"]))
        assert np.all(images["normal"][hit][:, 2] > 127) and not images["normal"][~hit][:, :3].any()     # facing the camera: blue
        assert images["depth"][hit][:, 0].min() >= 0 and images["depth"][hit][:, 0].max() == 255 and not images["depth"][~hit][:, :3].any()
        with pytest.raises(ValueError):
            viewer.renderMesh(mesh, "wireframe")
        path = tmp_path / "mesh.png"
        viewer.saveMeshPNG(str(path), mesh, "face")
        assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    finally:
        viewer.destroy()
