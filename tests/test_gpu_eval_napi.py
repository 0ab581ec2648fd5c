"""GPU: held-out evaluation through the node host (bindings/ts/trainer.js evaluate over the N-API addon, bindings/napi/eval_run.js) against the
Python host's on the same trained state: SSE, SSIM bit for bit, the split by loaders.holdoutSplit the same."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import loaders, ops

import harness
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("eval_entries", [0, 256])
def test_node_evaluate_equals_python_evaluate(hip_device, tmp_path, eval_entries):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, images = _views(dev, cfg, 12)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images, every=4)
    t = _trainer(dev, cfg, g, sh, trc, tri, pipeline_depth=2)
    t.setEvaluationViews(tec, tei)
    for _ in range(9):
        t.step()
    r_eval = t.evaluate()
    r_train = t.evaluate([3, 1], split="train")
    n = t.getPointCount()
    t.pointCloud.gaussian_3d_buffer.read(np.uint32, count=n * 6).tofile(tmp_path / "gaussians.bin")
    t.pointCloud.sh_buffer.read(np.uint32, count=n * 24).tofile(tmp_path / "sh.bin")   # (the read brings the deferred SH-DC halves in)
    np.stack([np.asarray(c["camera"], np.float32) for c in cameras]).tofile(tmp_path / "cameras.bin")
    np.concatenate([im["texture"].read(np.uint8) for im in images]).tofile(tmp_path / "images.bin")
    a, b = images[0]["texture"], images[1]["texture"]
    direct = (ops.imageSSE(dev, a, b, cfg.width * cfg.height), ops.imageSSIM(dev, a, b, cfg.width, cfg.height))
    t.destroy()
    (tmp_path / "meta.json").write_text(json.dumps(dict(num_points=n, sh_deg=cfg.sh_deg, sizes=[[im["width"], im["height"]] for im in images], every=4,
                                                        train_views=[3, 1], eval_max_tile_entries=eval_entries)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "eval_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "EVAL_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    hexf = lambda x: np.float64(x).tobytes().hex()
    assert out["split"] == [len(trc), len(tec)]
    for name, py in (("eval", r_eval), ("train", r_train)):
        js = out[name]
        assert js["views"] == py["views"]
        assert js["sse"] == py["sse"], f"{name}: SSE node {js['sse']} vs python {py['sse']}"
        assert js["ssim_hex"] == [hexf(x) for x in py["ssim"]], f"{name}: SSIM bits differ"
        assert abs(np.frombuffer(bytes.fromhex(js["mean_ssim_hex"]), np.float64)[0] - py["mean_ssim"]) <= 1e-15   # (the means: a host-side sum)
    assert out["direct"]["sse"] == direct[0] and out["direct"]["ssim_hex"] == hexf(direct[1])
    if eval_entries:
        assert "evaluation tile-entry lists grown" in r.stderr
