"""GPU: the normal maps through the node host (bindings/napi/normal_run.js over the N-API addon) and the Python host on the same synthetic scene: the
packed words, the composited image, the depth normals, the three agreement sums, the presentation bytes and Viewer.renderNormals byte for byte equal;
and the node Trainer's normalConsistency equal to the Python Trainer's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import images, ops, synth
from webdgs_amd.trainer import Trainer

import harness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_normal_maps_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20_000, width=320, height=240)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8)[3]
    n = cfg.width * cfg.height
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    dn, rgba = dev.createBuffer(16 * n), dev.createBuffer(4 * n)
    try:
        pipe.forward()
        pipe.rast.encodeNormal(None)
        pipe.rast.encodeDepth(None, ("median",))
        ops.depthToNormals(dev, pipe.rast.getDepthTextureView("median"), cfg.width, cfg.height, cam, dn)
        agreement = ops.normalAgreement(dev, pipe.rast.getNormalTextureView(), dn, cfg.width, cfg.height)
        ops.normalToRGBA8(dev, pipe.rast.getNormalTextureView(), cfg.width, cfg.height, rgba)
        py = dict(words=pipe.rast.getGaussianNormals().read(np.uint8)[:4 * cfg.num_points].tobytes(), normal=pipe.rast.getNormalTextureView().read(np.uint8).tobytes(),
                  depth_normals=dn.read(np.uint8).tobytes(), rgba=rgba.read(np.uint8).tobytes())
    finally:
        dn.destroy()
        rgba.destroy()
        pipe.destroy()
    # the Python Trainer's normalConsistency before any step: views 0 and 2 of the circle to train on, 5 and 6 held out (blank images: never looked at)
    cams = synth.circle_cameras(cfg, 8)
    train_views, eval_views = [0, 2], [5, 6]
    view = lambda v: dict(camera=cams[v], width=cfg.width, height=cfg.height)   # noqa: E731
    blank = lambda v: dict(texture=dev.bufferFrom(np.zeros(4 * n, np.uint8)), width=cfg.width, height=cfg.height)   # noqa: E731
    t = Trainer(dev, seed=5)
    try:
        t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
        t.setDataset([view(v) for v in train_views], [blank(v) for v in train_views])
        t.setEvaluationViews([view(v) for v in eval_views], [blank(v) for v in eval_views])
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.start()
        pick = lambda r: {k: r[k] for k in ("views", "sum_e", "sum_a", "pixels", "value", "mean", "iteration")}   # noqa: E731
        py_consistency = dict(eval_median=pick(t.normalConsistency()), train_expected=pick(t.normalConsistency([1, 0], "train", "expected")))
    finally:
        t.destroy()
    (tmp_path / "meta.json").write_text(json.dumps(dict(config=dict(config_id=cfg.config_id, num_points=cfg.num_points, width=cfg.width, height=cfg.height,
                                                                    sh_deg=cfg.sh_deg, fy=cfg.fy, s0=cfg.s0, name=cfg.name), cameras=8, view=3, train_views=train_views, eval_views=eval_views)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "normal_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NORMAL_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [] and out["render_mode"] == "pointcloud" and out["frame_unchanged"] is True and out["no_normal"] == ops.NO_NORMAL, out
    assert (tmp_path / "out_words.u32").read_bytes() == py["words"], "the packed per-Gaussian normals: node and python differ"
    assert (tmp_path / "out_normal.f32").read_bytes() == py["normal"], "the composited image: node and python differ"
    assert (tmp_path / "out_depth_normals.f32").read_bytes() == py["depth_normals"], "depthToNormals: node and python differ"
    assert (tmp_path / "out_rgba.rgba").read_bytes() == py["rgba"], "normalToRGBA8: node and python differ"
    assert (tmp_path / "out_viewer_normal.f32").read_bytes() == py["normal"], "Viewer.renderNormals (node) vs encodeNormal (python)"
    assert {k: out["agreement"][k] for k in ("sum_e", "sum_a", "pixels")} == {k: agreement[k] for k in ("sum_e", "sum_a", "pixels")}
    assert out["agreement"]["value"] == agreement["value"] and agreement["pixels"] > 0
    assert out["consistency"] == py_consistency, "Trainer.normalConsistency: node and python differ"
    assert all(p > 0 for p in py_consistency["eval_median"]["pixels"] + py_consistency["train_expected"]["pixels"]) and py_consistency["train_expected"]["views"] == [1, 0]
    png = images.decodePNG((tmp_path / "out_viewer_normal.png").read_bytes())
    assert png.tobytes() == py["rgba"], "Viewer.saveNormalPNG (node) decodes to the kernel's bytes"
