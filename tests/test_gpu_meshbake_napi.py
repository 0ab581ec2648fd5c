"""GPU: vertex colours baked from photographs through the node host (bindings/napi/meshbake_run.js over the N-API addon): SHA-256 digests of the state, the
colours, the mask and the totals of every crafted case equal to the restatement's (tests/meshbake_ref.py) -- which tests/test_gpu_meshbake.py holds the Python
host to -- the icosphere through bakeVertexColours with and without occlusion, and Trainer.bakeMeshColours of both hosts on one cloud, dataset and mesh."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops

import harness
import meshbake_ref as B
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
    want = dict(cases={})
    # 1. the crafted cases
    for name in sorted(B.CASES):
        m = B.case(name)
        m["vertices"].tofile(str(tmp_path / f"{name}.vertices.f32"))
        for key in ("normals", "fallback"):
            if m[key] is not None:
                m[key].tofile(str(tmp_path / f"{name}.{key}.{'f32' if key == 'normals' else 'u8'}"))
        views = []
        for k, w in enumerate(m["views"]):
            w["camera"].tofile(str(tmp_path / f"{name}.{k}.camera.f32"))
            w["image"].tofile(str(tmp_path / f"{name}.{k}.image.u8"))
            if w["depth"] is not None:
                w["depth"].tofile(str(tmp_path / f"{name}.{k}.depth.f32"))
            views.append(dict(width=w["width"], height=w["height"], near=w["near"], depth_tolerance=w["depth_tolerance"], min_cos=w["min_cos"], depth=w["depth"] is not None))
        meta["cases"].append(dict(name=name, vertices=int(m["vertices"].shape[0]), normals=m["normals"] is not None, fallback=m["fallback"] is not None, views=views,
                                  min_views=m["min_views"], min_weight=m["min_weight"]))
        want["cases"][name] = B.digest(B.expected(name))
    # 2. the icosphere under the rolled, the steep and the close camera: the Python host's results, which test_gpu_meshbake.py holds to the restatement
    spheres = [B.sphere(name) for name in B.SPHERE_CAMERAS]
    s0 = spheres[0]
    for key, suffix in (("vertices", "f32"), ("faces", "u32"), ("colours", "u8"), ("normals", "f32")):
        s0[key].tofile(str(tmp_path / f"sphere.{key}.{suffix}"))
    np.stack([s["camera"] for s in spheres]).astype(np.float32).tofile(str(tmp_path / "sphere.cameras.f32"))
    np.stack([s["image"] for s in spheres]).tofile(str(tmp_path / "sphere.images.u8"))
    meta["sphere"] = dict(width=s0["width"], height=s0["height"], near=s0["near"], depth_tolerance=0.0625, min_cos=0.1)
    mesh = dict(vertices=s0["vertices"], faces=s0["faces"], colours=s0["colours"], normals=s0["normals"])
    want["sphere"] = {}
    for what, occlusion in (("occlusion", True), ("plain", False)):
        r = ops.bakeVertexColours(dev, mesh, [s["camera"] for s in spheres], [s["image"] for s in spheres], s0["width"], s0["height"], depthTolerance=0.0625, minCos=0.1,
                                  near=s0["near"], occlusion=occlusion)
        want["sphere"][what] = dict(colours=sha(r["colours"]), baked=sha(r["baked"].astype(np.uint8)), stats=r["stats"])
    assert want["sphere"]["occlusion"]["stats"]["bakedVertices"] < want["sphere"]["plain"]["stats"]["bakedVertices"]
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
        baked = t.bakeMeshColours(fused, depthTolerance=voxel)
        few = t.bakeMeshColours(fused, depthTolerance=voxel, viewIds=[2], normals=False, occlusion=False)
        n = t.getPointCount()
        t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
        t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
    finally:
        t.destroy()
    assert 0 < baked["stats"]["bakedVertices"] < fused["vertices"].shape[0]
    np.stack([np.asarray(c["camera"], np.float32) for c in views]).tofile(tmp_path / "cameras.bin")
    np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
    for key, suffix in (("vertices", "f32"), ("faces", "u32"), ("colours", "u8")):
        np.ascontiguousarray(fused[key]).tofile(str(tmp_path / f"fused.{key}.{suffix}"))
    meta["trainer"] = dict(num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], depth_tolerance=voxel)
    want["trainer"] = dict(views=baked["views"], colours=sha(baked["colours"]), baked=sha(baked["baked"].astype(np.uint8)), stats=baked["stats"], fewViews=few["views"],
                           fewColours=sha(few["colours"]), fewStats=few["stats"])
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshbake_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHBAKE_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["cases"]:
        assert out["cases"][name] == want["cases"][name], name
    assert out["sphere"] == want["sphere"], (out["sphere"], want["sphere"])
    assert out["trainer"] == want["trainer"], (out["trainer"], want["trainer"])
