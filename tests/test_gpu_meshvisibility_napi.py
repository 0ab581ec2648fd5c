"""GPU: per-face visibility, its rule and the face filter through the node host (bindings/napi/meshvisibility_run.js over the N-API addon): SHA-256 digests of
the counters of the crafted face images, of the flags of a set of rules, of meshes filtered under crafted masks and of the culled icosphere, equal to the
restatement's (tests/meshvisibility_ref.py) -- which tests/test_gpu_meshvisibility.py holds the Python host to -- and Trainer.meshVisibility and
Trainer.cullMesh of both hosts on one cloud, dataset and mesh."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import harness
import meshclean_ref as M
import meshraster_ref as R
import meshvisibility_ref as VR
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [dict(), dict(minPixels=0, minViews=0), dict(minPixels=7, minViews=2), dict(minAgreeing=3), dict(minAgreeingFraction=0.5), dict(minAgreeingFraction=1.0 / 3.0),
         dict(minPixels=2, minViews=1, minAgreeing=1, minAgreeingFraction=1.0)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def mesh_digest(m):
    return sha(m["vertices"], m["faces"], m["vertexMap"], m["faceMap"])


def _depths(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 5.0, n).astype(np.float32)
    b = (a + rng.uniform(-0.1, 0.1, n).astype(np.float32)).astype(np.float32)
    b[rng.integers(0, 6, n) == 0] = 0.0
    return a, b, rng.uniform(0.0, 1.0, n).astype(np.float32)


def test_node_digests_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    meta = dict(images=[], rules=RULES, masks=[])
    want = dict(images={}, masks={})
    # 1. the crafted images
    for name in sorted(VR.IMAGES):
        F, w, h, img = VR.image(name)
        a, b, ws = _depths(img.size, 13)
        for suffix, x in (("face.u32", img), ("a.f32", a), ("b.f32", b), ("ws.f32", ws)):
            x.tofile(str(tmp_path / f"{name}.{suffix}"))
        ref = VR.Accumulator(F)
        ref.accumulate(img, a, b, ws, 0.5, 0.05)
        ref.accumulate(img)
        meta["images"].append(dict(name=name, faces=F, width=w, height=h, min_weight_sum=0.5, threshold=0.05))
        want["images"][name] = dict(counters=sha(ref.counters), stats=ref.stats())
    # 2. the rule
    rng = np.random.default_rng(41)
    pixels = rng.integers(0, 50, 3000)
    counters = np.stack([pixels, rng.integers(0, 51, 3000) * pixels // 50, rng.integers(0, 5, 3000)], axis=1).astype(np.uint32)
    counters[:4] = [[10, 5, 2], [65536, 21845, 1], [2 ** 32 - 1, 2 ** 32 - 2, 1], [0, 0, 0]]
    counters.tofile(str(tmp_path / "counters.u32"))
    flags = [sha(VR.flags(counters, r.get("minPixels", 1), r.get("minViews", 1), r.get("minAgreeing", 0), VR.fraction_q16(r.get("minAgreeingFraction", 0.0)))) for r in RULES]
    want["rules"] = [dict(device=f, host=f) for f in flags]
    # 3. the filter
    faces, V, _ = M.shape("clusters")
    mesh = M.as_mesh(faces, V)
    mesh["vertices"].tofile(str(tmp_path / "mesh.vertices.f32"))
    mesh["faces"].tofile(str(tmp_path / "mesh.faces.u32"))
    nf = faces.shape[0]
    valid = np.all(faces.astype(np.int64) < V, axis=1)
    masks = {"ones": np.ones(nf, np.uint8), "zeros": np.zeros(nf, np.uint8), "alternate": (np.arange(nf) % 2 == 0).astype(np.uint8), "invalid": (~valid).astype(np.uint8),
             "random": (np.random.default_rng(3).integers(0, 4, nf) == 0).astype(np.uint8)}
    for name, keep in masks.items():
        keep.tofile(str(tmp_path / f"{name}.keep.u8"))
        meta["masks"].append(name)
        f = VR.filter_faces(mesh, keep)
        want["masks"][name] = dict(host=mesh_digest(f), device=mesh_digest(f), vertices=int(f["vertexMap"].size), faces=int(f["faceMap"].size), invalidFaces=f["invalidFaces"])
    # 4. the icosphere under the rolled, the steep and the close camera
    m = R.case("sphere-roll37")
    cameras = [R.case(name)["camera"] for name in ("sphere-roll37", "sphere-below", "sphere-close")]
    m["vertices"].tofile(str(tmp_path / "sphere.vertices.f32"))
    m["faces"].tofile(str(tmp_path / "sphere.faces.u32"))
    np.stack(cameras).astype(np.float32).tofile(str(tmp_path / "sphere.cameras.f32"))
    meta["sphere"] = dict(width=m["width"], height=m["height"], near=m["near"])
    ref = VR.Accumulator(m["faces"].shape[0])
    for r in (R.expected("sphere-roll37"), R.expected("sphere-below"), R.rasterize(m["vertices"], m["faces"], None, cameras[2], m["width"], m["height"], m["near"])):
        ref.accumulate(r["face"])
    culled = VR.filter_faces(m, VR.flags(ref.counters))
    want["sphere"] = dict(counters=sha(ref.counters), stats=ref.stats(), culled=mesh_digest(culled), faces=int(culled["faceMap"].size))
    # 5. the Trainer surface: the Python host's results on one cloud, dataset and mesh
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh_, views, images = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh_, views, images, densify=False)
    voxel, rule = 0.11, dict(minPixels=2, minAgreeingFraction=0.25)
    try:
        for _ in range(4):
            t.step()
        t.drain()
        fused = t.extractMesh((-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), voxel)
        vis = t.meshVisibility(fused, threshold=voxel)
        cut = t.cullMesh(fused, threshold=voxel, **rule)
        n = t.getPointCount()
        t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
        t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
    finally:
        t.destroy()
    assert sum(vis["counted"]) > 0 and 0 < cut["faces"].shape[0] < fused["faces"].shape[0]
    np.stack([np.asarray(c["camera"], np.float32) for c in views]).tofile(tmp_path / "cameras.bin")
    np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
    fused["vertices"].tofile(str(tmp_path / "fused.vertices.f32"))
    fused["faces"].tofile(str(tmp_path / "fused.faces.u32"))
    meta["trainer"] = dict(num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], threshold=voxel, rule=rule)
    want["trainer"] = dict(views=vis["views"], counters=sha(vis["counters"]), counted=vis["counted"], agreeing=vis["agreeing"], foreign=vis["foreign"], iteration=None,
                           culled=mesh_digest(cut), culledCounters=sha(cut["counters"]), faces=int(cut["faces"].shape[0]))
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshvisibility_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHVISIBILITY_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["images"]:
        assert out["images"][name] == want["images"][name], (name, out["images"][name], want["images"][name])
    assert out["rules"] == want["rules"]
    for name in want["masks"]:
        assert out["masks"][name] == want["masks"][name], (name, out["masks"][name], want["masks"][name])
    assert out["sphere"] == want["sphere"], (out["sphere"], want["sphere"])
    got = dict(out["trainer"], iteration=None)   # (the node trainer starts from the saved cloud: its iteration counter is its own)
    assert got == want["trainer"], (got, want["trainer"])
