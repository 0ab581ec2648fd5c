"""GPU: per-Gaussian contribution and contribution-based pruning through the node host (bindings/napi/contrib_run.js over the N-API addon) against the
Python host's, on the big-splats scene of test_gpu_contrib (ops level) and on a trained Trainer: the records and the pruned cloud, sha256 equal."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import synth

import harness
from test_depth_reference import scene_config
from test_gpu_contrib import TRAINER_CFG, prune_never_composited
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def _node(tmp_path, meta):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "contrib_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONTRIB_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out
    return out, lambda name: (tmp_path / name).read_bytes()


def test_node_records_and_pruned_scene_equal_the_python_hosts(hip_device, tmp_path):
    cfg = scene_config("big-splats")
    g, sh, _ = harness.scene(cfg)
    rec, actions, counts, total, new_g, new_sh, _ = prune_never_composited(hip_device, cfg, g, sh, synth.circle_cameras(cfg, 3))
    out, read = _node(tmp_path, dict(mode="scene", cameras=3, config=dict(config_id=cfg.config_id, num_points=cfg.num_points, width=cfg.width, height=cfg.height,
                                                                         sh_deg=cfg.sh_deg, fy=cfg.fy, s0=cfg.s0, name=cfg.name)))
    assert out["total"] == total and 0 < total < cfg.num_points
    assert sha(read("out_stats.bin")) == sha(rec), "the statistics buffer: node and python differ"
    assert sha(read("out_gaussians.bin"), read("out_sh.bin")) == sha(new_g, new_sh), "the pruned cloud: node and python differ"


def test_node_trainer_prune_equals_the_python_hosts(hip_device, tmp_path):
    dev = hip_device
    cfg = harness.small_config(**TRAINER_CFG)
    g, sh, cameras, images = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, images, densify=False)
    try:
        for _ in range(20):
            t.step()
        n = t.getPointCount()
        t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
        t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
        np.stack([np.asarray(c["camera"], np.float32) for c in cameras]).tofile(tmp_path / "cameras.bin")
        np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
        stats, some = t.contributionStats(), t.contributionStats([2, 1])
        r = t.pruneByContribution(minPixels=1)
        m = t.getPointCount()
        py_g = t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=m * 6)
        py_sh = t.pointCloud.sh_buffer.read(np.uint32, count=m * 24)
        sse = t.evaluate(split="train")["sse"]
    finally:
        t.destroy()
    out, read = _node(tmp_path, dict(mode="trainer", num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], some_views=[2, 1]))
    assert out["result"] == r and out["points"] == m and r["pruned"] > 0 and out["views"] == stats["views"] and out["some_views"] == [2, 1]
    assert sha(read("out_sum_q.bin"), read("out_max_weight.bin"), read("out_pixels.bin")) == sha(stats["sum_q"], stats["max_weight"], stats["pixels"]), \
        "contributionStats: node and python differ"
    assert sha(read("out_some_pixels.bin")) == sha(some["pixels"])
    assert sha(read("out_gaussians.bin"), read("out_sh.bin")) == sha(py_g, py_sh), "the pruned cloud: node and python differ"
    assert out["sse"] == sse
