"""GPU: a texture atlas baked from photographs through the node host (bindings/napi/meshtexture_run.js over the N-API addon): SHA-256 digests of the rows, the
texture, the texel states and the totals of every crafted case equal to the restatement's (tests/meshtexture_ref.py) -- which tests/test_gpu_meshtexture.py
holds the Python host to -- the layout's texture coordinates byte for byte, the icosphere through bakeTexture with and without occlusion, Trainer.bakeMeshTexture and extractMesh(texture=...) of both hosts on one cloud, dataset and mesh, and the OBJ, MTL and PNG files of both hosts byte for byte."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import loaders, ops

import harness
import meshtexture_ref as T
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_node_digests_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    meta = dict(cases=[])
    want = dict(cases={}, layouts={})
    # 1. the crafted cases
    for name in sorted(T.CASES):
        m = T.case(name)
        m["vertices"].tofile(str(tmp_path / f"{name}.vertices.f32"))
        m["faces"].tofile(str(tmp_path / f"{name}.faces.u32"))
        if m["colours"] is not None:
            m["colours"].tofile(str(tmp_path / f"{name}.colours.u8"))
        views = []
        for k, w in enumerate(m["views"]):
            w["camera"].tofile(str(tmp_path / f"{name}.{k}.camera.f32"))
            w["image"].tofile(str(tmp_path / f"{name}.{k}.image.u8"))
            if w["depth"] is not None:
                w["depth"].tofile(str(tmp_path / f"{name}.{k}.depth.f32"))
            views.append(dict(width=w["width"], height=w["height"], near=w["near"], depth_tolerance=w["depth_tolerance"], min_cos=w["min_cos"], two_sided=w["two_sided"],
                              depth=w["depth"] is not None))
        F = int(m["faces"].shape[0])
        meta["cases"].append(dict(name=name, vertices=int(m["vertices"].shape[0]), faces=F, cell=m["cell"], colours=m["colours"] is not None, views=views,
                                  min_weight=m["min_weight"], fill=m["fill"]))
        want["cases"][name] = T.digest(T.expected(name))
        want["layouts"][name] = sha(ops.textureLayout(F, m["cell"])["uv"])
    # 2. the icosphere under the rolled, the steep and the close camera: the Python host's results, which test_gpu_meshtexture.py holds to the restatement
    spheres = [T.sphere(name) for name in T.SPHERE_CAMERAS]
    s0 = spheres[0]
    for key, suffix in (("vertices", "f32"), ("faces", "u32"), ("colours", "u8")):
        s0[key].tofile(str(tmp_path / f"sphere.{key}.{suffix}"))
    np.stack([s["camera"] for s in spheres]).astype(np.float32).tofile(str(tmp_path / "sphere.cameras.f32"))
    np.stack([s["image"] for s in spheres]).tofile(str(tmp_path / "sphere.images.u8"))
    meta["sphere"] = dict(width=s0["width"], height=s0["height"], near=s0["near"], depth_tolerance=0.0625, min_cos=0.1, cell=16)
    mesh = dict(vertices=s0["vertices"], faces=s0["faces"], colours=s0["colours"])
    want["sphere"] = {}
    for what, occlusion in (("occlusion", True), ("plain", False)):
        r = ops.bakeTexture(dev, mesh, [s["camera"] for s in spheres], [s["image"] for s in spheres], s0["width"], s0["height"], cell=16, depthTolerance=0.0625, minCos=0.1,
                            near=s0["near"], occlusion=occlusion)
        if occlusion:
            os.makedirs(tmp_path / "py")
            loaders.saveMeshOBJ(str(tmp_path / "py" / "mesh.obj"), r)
        want["sphere"][what] = dict(texture=sha(r["texture"]), state=sha(r["texelState"]), uv=sha(r["uv"]), size=[r["textureWidth"], r["textureHeight"]],
                                    stats=r["textureStats"])
    want_size = want["sphere"]["occlusion"]["size"]
    assert want["sphere"]["occlusion"]["stats"]["bakedTexels"] < want["sphere"]["plain"]["stats"]["bakedTexels"]
    # 3. the Trainer surface: the Python host's results on one cloud, dataset and mesh
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh_, views, images = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh_, views, images, densify=False)
    voxel = 0.11
    try:
        for _ in range(4):
            t.step()
        t.drain()
        fused = t.extractMesh((-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), voxel)
        baked = t.bakeMeshTexture(fused, depthTolerance=voxel, cell=4)
        few = t.bakeMeshTexture(fused, depthTolerance=voxel, viewIds=[2], occlusion=False, fill=False)
        ex = t.extractMesh((-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), voxel, texture=dict(depthTolerance=voxel, cell=4))
        n = t.getPointCount()
        t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
        t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
    finally:
        t.destroy()
    assert 0 < baked["textureStats"]["bakedTexels"] and few["textureStats"]["filledTexels"] == 0
    np.stack([np.asarray(c["camera"], np.float32) for c in views]).tofile(tmp_path / "cameras.bin")
    np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
    for key, suffix in (("vertices", "f32"), ("faces", "u32"), ("colours", "u8")):
        np.ascontiguousarray(fused[key]).tofile(str(tmp_path / f"fused.{key}.{suffix}"))
    meta["trainer"] = dict(num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], depth_tolerance=voxel, lo=[-2.01, -1.52, 2.03],
                           hi=[2.0, 1.5, 9.0], voxel=voxel)
    extracted = dict(vertices=sha(ex["vertices"]), faces=sha(ex["faces"]), texture=sha(ex["texture"]), uv=sha(ex["uv"]), stats=ex["textureStats"], views=ex["views"])
    assert_bits_equal(ex["texture"], baked["texture"], "extractMesh(texture) on the raw mesh is bakeMeshTexture of it")
    want["trainer"] = dict(views=baked["views"], texture=sha(baked["texture"]), state=sha(baked["texelState"]), stats=baked["textureStats"], fewViews=few["views"],
                           fewTexture=sha(few["texture"]), fewStats=few["textureStats"], extracted=extracted)
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshtexture_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHTEXTURE_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["cases"]:
        assert out["cases"][name] == want["cases"][name], name
        assert out["layouts"][name] == want["layouts"][name], name
    assert out["sphere"] == want["sphere"], (out["sphere"], want["sphere"])
    assert out["trainer"] == want["trainer"], (out["trainer"], want["trainer"])
    for name in ("mesh.obj", "mesh.mtl", "mesh.png"):   # the node host's OBJ writer gives the Python host's bytes
        assert (tmp_path / "js" / name).read_bytes() == (tmp_path / "py" / name).read_bytes(), name
    back = loaders.loadMeshOBJ(str(tmp_path / "js" / "mesh.obj"))
    assert back["texture"].shape == (want_size[1], want_size[0], 4) and back["uv"].tobytes() == ops.textureLayout(int(s0["faces"].shape[0]), 16)["uv"].tobytes()
