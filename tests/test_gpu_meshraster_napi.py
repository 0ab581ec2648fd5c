"""GPU: the mesh rasterizer and the depth agreement through the node host (bindings/napi/meshraster_run.js over the N-API addon) on the crafted cases of
tests/meshraster_ref.py: SHA-256 digests of every image and the statistics, equal to the restatement's -- which tests/test_gpu_meshraster.py holds the Python
host to -- and Trainer.meshDepthAgreement of both hosts on one cloud, dataset and mesh."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import harness
import meshraster_ref as R
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_images_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    meta = dict(cases=[], agreement=[])
    want = dict(cases={}, agreement={})
    for name in sorted(R.CASES):
        m, e = R.case(name), R.expected(name)
        m["vertices"].tofile(str(tmp_path / f"{name}.vertices.f32"))
        m["faces"].tofile(str(tmp_path / f"{name}.faces.u32"))
        m["camera"].tofile(str(tmp_path / f"{name}.camera.f32"))
        if m["colours"] is not None:
            m["colours"].tofile(str(tmp_path / f"{name}.colours.u8"))
        meta["cases"].append(dict(name=name, colours=m["colours"] is not None, width=m["width"], height=m["height"], near=m["near"], cull=m["cull"]))
        want["cases"][name] = dict(device=R.digest(e), host=R.digest(e), stats=e["stats"])
    for name, c in sorted(R.AGREEMENT_CASES.items()):
        c["a"].tofile(str(tmp_path / f"{name}.a.f32"))
        c["b"].tofile(str(tmp_path / f"{name}.b.f32"))
        if c["weight_sum"] is not None:
            c["weight_sum"].tofile(str(tmp_path / f"{name}.ws.f32"))
        meta["agreement"].append(dict(name=name, weight_sum=c["weight_sum"] is not None, min_weight_sum=c["min_weight_sum"], width=c["width"], height=c["height"],
                                      max_difference=c["max_difference"], threshold=c["threshold"]))
        want["agreement"][name] = R.agreement_expected(name)
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshraster_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHRASTER_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["cases"]:
        assert out["cases"][name] == want["cases"][name], (name, out["cases"][name], want["cases"][name])
    assert out["agreement"] == want["agreement"], (out["agreement"], want["agreement"])


def test_node_mesh_depth_agreement_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, images, densify=False)
    voxel = 0.11
    try:
        for _ in range(4):
            t.step()
        t.drain()
        mesh = t.extractMesh((-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), voxel)
        want = t.meshDepthAgreement(mesh, split="train", maxDifference=1.0, threshold=voxel)
        n = t.getPointCount()
        t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
        t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
    finally:
        t.destroy()
    assert sum(want["both"]) > 0
    np.stack([np.asarray(c["camera"], np.float32) for c in cameras]).tofile(tmp_path / "cameras.bin")
    np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
    mesh["vertices"].tofile(str(tmp_path / "mesh.vertices.f32"))
    mesh["faces"].tofile(str(tmp_path / "mesh.faces.u32"))
    meta = dict(cases=[], agreement=[], trainer=dict(num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], max_difference=1.0,
                                                     threshold=voxel))
    R.case("nothing")["camera"].tofile(str(tmp_path / "nothing.camera.f32"))
    meta["cases"].append(dict(name="nothing", colours=False, width=8, height=8, near=0.01, cull="none"))
    for k in ("vertices.f32", "faces.u32"):
        (tmp_path / f"nothing.{k}").write_bytes(b"")
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshraster_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHRASTER_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    got = out["trainer"]
    for k in ("views", "both", "onlyA", "onlyB", "within", "sum_q"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("both", "onlyA", "onlyB", "within", "sum_q"):
        assert got["total"][k] == want["total"][k]
    assert got["last"] == [want[k][-1] for k in ("both", "onlyA", "onlyB", "within", "sum_q")]
