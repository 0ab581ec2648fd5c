"""GPU: the exact D-SSIM loss through the node host -- bindings/ts/trainer.js over the N-API addon with trainingConfig.dssim_mode = 'gaussian'
(bindings/napi/trainer_run.js) against the Python host on the same dataset and view draws: cloud and the six optimizer-state arrays bit for bit
after a run across a densify event, and the JS binding's validation of the mode."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops, synth
from webdgs_amd.trainer import Trainer

import harness
from harness import assert_bits_equal
from test_gpu_trainer_oracle import _FixedViews

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _node():
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    return node


@pytest.mark.parametrize("form", [dict(), dict(views_per_step=2, lanes=2, pipeline_depth=2)], ids=["one_view", "batched_two_lanes_depth2"])
def test_node_trainer_gaussian_loss_equals_python(hip_device, orc, tmp_path, form):
    node = _node()
    dev = hip_device
    vps = form.get("views_per_step", 1)
    cfg = harness.small_config("c2", num_points=5000, width=128, height=96, s0=0.01)
    g, sh, _ = harness.scene(cfg)
    tg, tsh = synth.make_target_scene(g, sh)
    cams = synth.circle_cameras(cfg, 4)
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    imgs = [orc.forward(tg, tsh, cams[i], st, ti)["rgba8"] for i in range(4)]
    dens = dict(schedule=dict(enabled=True, warmupIterations=6, interval=50, stopIterations=40), metricViews=3, metricDownscale=2, metricThreshold=0.5,
                cloneThresholdCount=5, splitScaleThreshold=0.03, pruneOpacity=0.2, maxNewPointsPerStep=300, maxBufferBytes=128 * 1024 * 1024)
    steps = 9
    train_views, second, metric_views = [2, 0, 3, 1, 1, 2, 0, 3, 2], [1, 3, 0, 2, 3, 3, 1, 0, 0], {6: [1, 3, 0]}
    draws = []
    for i in range(steps):
        draws.append(train_views[i])
        if vps == 2:
            draws.append(second[i])
        draws += metric_views.get(i + 1, [])
    tc = dict(dssim_mode="gaussian")
    g.tofile(tmp_path / "gaussians.bin")
    sh.tofile(tmp_path / "sh.bin")
    np.ascontiguousarray(cams, np.float32).tofile(tmp_path / "cameras.bin")
    np.stack(imgs).tofile(tmp_path / "images.bin")
    (tmp_path / "meta.json").write_text(json.dumps(dict(num_points=cfg.num_points, sh_deg=cfg.sh_deg, width=cfg.width, height=cfg.height, views=4, steps=steps,
                                                        draws=draws, densify=dens, training_config=tc, **form)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "trainer_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TRAINER_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out_meta.json").read_text())

    t = Trainer(dev, trainingConfig=tc, seed=0, views_per_rank=vps, overlap_views=form.get("lanes"), pipeline_depth=form.get("pipeline_depth", 1))
    t.setDensifyPruneConfig(dens)
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset([dict(camera=cams[i], width=cfg.width, height=cfg.height) for i in range(4)],
                 [dict(texture=dev.bufferFrom(imgs[i]), width=cfg.width, height=cfg.height) for i in range(4)])
    t.start()
    t._rng = _FixedViews(draws)
    try:
        for _ in range(steps):
            t.step()
        dev.synchronize()
        n = t.getPointCount()
        assert out["num_points"] == n and out["iteration"] == t.getIteration() == steps
        assert_bits_equal(np.fromfile(tmp_path / "out_gaussians.bin", np.uint32), t.pointCloud.gaussian_3d_buffer.read(np.uint32)[: n * 6], "node vs python: gaussians")
        assert_bits_equal(np.fromfile(tmp_path / "out_sh.bin", np.uint32), t.pointCloud.sh_buffer.read(np.uint32)[: n * 24], "node vs python: sh")
        words = dict(optPosBuffer=12, optRotBuffer=12, optScaleBuffer=12, optOpacityBuffer=3, paramSH=48, stateSH=96)
        for k, b in t.optimizer.getStateBuffers().items():
            assert_bits_equal(np.fromfile(tmp_path / f"out_state_{k}.bin", np.uint32), b.read(np.uint32)[: n * words[k]], f"node vs python: state {k}")
    finally:
        t.destroy()


def test_node_binding_validates_the_mode(tmp_path):
    node = _node()
    script = tmp_path / "mode.js"
    script.write_text(f"""'use strict';
const hip = require({json.dumps(os.path.join(ROOT, 'bindings', 'ts', 'webdgs_hip.js'))});
const dev = new hip.HipDevice(0);
const upload = (n) => {{ const b = dev.createBuffer({{ size: n }}); dev.queue.writeBuffer(b, 0, new Uint8Array(n)); return b; }};
const pc = {{ type: 'full', num_points: 1, sh_deg: 0, gaussian_3d_buffer: upload(24), sh_buffer: upload(96) }};
const cfg = (m) => ({{ viewportWidth: 8, viewportHeight: 8, trainingConfig: {{ lambda_l1: 0.8, lambda_l2: 0, lambda_dssim: 0.2, dssim_mode: m }} }});
let refused = 0;
try {{ new hip.TiledBackwardPass(dev, pc, cfg('box')); }} catch (e) {{ refused++; }}
const p = new hip.TiledBackwardPass(dev, pc, cfg('gaussian'));
try {{ p.setTrainingConfig({{ dssim_mode: 3 }}); }} catch (e) {{ refused++; }}
const kept = p.trainingConfig.dssim_mode;
p.setTrainingConfig({{ dssim_mode: 'reference' }});
console.log(JSON.stringify({{ refused, kept, now: p.trainingConfig.dssim_mode }}));
p.destroy();
dev.synchronize();
""")
    r = subprocess.run([node, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == dict(refused=2, kept="gaussian", now="reference")
