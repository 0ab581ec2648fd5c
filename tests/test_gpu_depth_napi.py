"""GPU: the depth images through the node host (bindings/napi/depth_run.js over the N-API addon) and the Python host on the same synthetic scene:
the three images, the presentation bytes and Viewer.renderDepth byte for byte equal."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops, synth

import harness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_depth_images_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20_000, width=320, height=240)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8)[3]
    near, far = 2.5, 9.0
    pipe = harness.HipPipeline(dev, cfg, g, sh, cam)
    try:
        pipe.forward()
        pipe.rast.encodeDepth(None, ("expected", "median", "weight_sum"))
        grey = dev.createBuffer(4 * cfg.width * cfg.height)
        ops.depthToRGBA8(dev, pipe.rast.getDepthTextureView("expected"), cfg.width, cfg.height, near, far, grey)
        py = {k: pipe.rast.getDepthTextureView(k).read(np.uint8).tobytes() for k in ops.DEPTH_KINDS}
        py["alpha"] = pipe.rast.getAlphaTextureView().read(np.uint8).tobytes()
        py_grey = grey.read(np.uint8).tobytes()
        grey.destroy()
    finally:
        pipe.destroy()
    (tmp_path / "meta.json").write_text(json.dumps(dict(config=dict(config_id=cfg.config_id, num_points=cfg.num_points, width=cfg.width, height=cfg.height,
                                                                    sh_deg=cfg.sh_deg, fy=cfg.fy, s0=cfg.s0, name=cfg.name), cameras=8, view=3, near=near, far=far)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "depth_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEPTH_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [] and out["render_mode"] == "pointcloud" and out["frame_unchanged"] is True, out
    for k in ops.DEPTH_KINDS:
        assert (tmp_path / f"out_{k}.f32").read_bytes() == py[k], f"{k}: node and python differ"
    assert (tmp_path / "out_alpha.f32").read_bytes() == py["alpha"]
    assert (tmp_path / "out_grey.rgba").read_bytes() == py_grey, "depthToRGBA8: node and python differ"
    assert (tmp_path / "out_viewer_median.f32").read_bytes() == py["median"], "Viewer.renderDepth (node) vs encodeDepth (python)"
    assert np.frombuffer(py["median"], np.float32).max() > 0
