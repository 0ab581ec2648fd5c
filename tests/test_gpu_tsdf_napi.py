"""GPU: TSDF fusion and mesh extraction through the node host (bindings/napi/tsdf_run.js over the N-API addon) and the Python host on the same
synthetic scene: the volume's tsdf / weight / rgb, the triangle buffers and the saved PLY byte for byte equal, and the node Trainer's fuseDepth equal
to the Python Trainer's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import loaders, ops, synth
from webdgs_amd.trainer import Trainer

import harness
from test_gpu_tsdf import SCENE_DIMS, SCENE_ORIGIN, SCENE_VOXEL, _read_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_tsdf_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cfg = harness.small_config("c2", num_points=20_000, width=320, height=240)
    g, sh = synth.make_gaussians(cfg)
    cams = synth.circle_cameras(cfg, 4)
    pipe = harness.HipPipeline(dev, cfg, g, sh, cams[0])
    vol = ops.TSDFVolume(dev, SCENE_ORIGIN, SCENE_VOXEL, SCENE_DIMS)
    try:
        for c in cams:
            pipe.camera.write(c)
            pipe.forward()
            pipe.rast.encodeDepth(None, ("median", "weight_sum"))
            vol.integrate(pipe.rast.getDepthTextureView("median"), pipe.camera, cfg.width, cfg.height, weightSum=pipe.rast.getDepthTextureView("weight_sum"),
                          colour=pipe.rast.getOutputTextureView())
        T, W, rgb = _read_volume(vol)
        tri = vol.extractTriangles()
        mesh = vol.extractMesh()
        loaders.saveMeshPLY(str(tmp_path / "py_mesh.ply"), mesh)
        truncation = vol.truncation
    finally:
        vol.destroy()
        pipe.destroy()
    assert tri["keys"].shape[0] > 0 and (W > 0).any()
    # the Python Trainer's fuseDepth before any step (blank images: never looked at)
    n = cfg.width * cfg.height
    train_views, fuse_order = [0, 1, 3], [2, 0]
    t = Trainer(dev, seed=5)
    tvol = ops.TSDFVolume(dev, SCENE_ORIGIN, SCENE_VOXEL, SCENE_DIMS)
    try:
        t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
        t.setDataset([dict(camera=cams[v], width=cfg.width, height=cfg.height) for v in train_views],
                     [dict(texture=dev.bufferFrom(np.zeros(4 * n, np.uint8)), width=cfg.width, height=cfg.height) for _ in train_views])
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.start()
        assert t.fuseDepth(tvol, fuse_order) == fuse_order
        tT, _, trgb = _read_volume(tvol)
    finally:
        tvol.destroy()
        t.destroy()
    (tmp_path / "meta.json").write_text(json.dumps(dict(config=dict(config_id=cfg.config_id, num_points=cfg.num_points, width=cfg.width, height=cfg.height,
                                                                    sh_deg=cfg.sh_deg, fy=cfg.fy, s0=cfg.s0, name=cfg.name), cameras=4,
                                                        origin=[float(np.float32(x)) for x in SCENE_ORIGIN], voxel_size=SCENE_VOXEL, dims=list(SCENE_DIMS),
                                                        train_views=train_views, fuse_order=fuse_order)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "tsdf_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TSDF_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [] and out["empty_count"] == 0 and out["dims"] == list(SCENE_DIMS) and out["fused"] == fuse_order, out
    assert out["triangles"] == tri["keys"].shape[0] and out["vertices"] == mesh["vertices"].shape[0] and out["truncation"] == truncation and out["trainer_mesh_faces"] > 0
    assert (tmp_path / "out_tsdf.f32").read_bytes() == T.tobytes(), "tsdf: node and python differ"
    assert (tmp_path / "out_weight.f32").read_bytes() == W.tobytes(), "weight: node and python differ"
    assert (tmp_path / "out_rgb.f32").read_bytes() == rgb.tobytes(), "rgb: node and python differ"
    assert (tmp_path / "out_positions.f32").read_bytes() == tri["positions"].tobytes(), "triangle positions: node and python differ"
    assert (tmp_path / "out_keys.u64").read_bytes() == tri["keys"].tobytes(), "triangle keys: node and python differ"
    assert (tmp_path / "out_colours.rgba").read_bytes() == tri["colours"].tobytes(), "triangle colours: node and python differ"
    assert (tmp_path / "out_mesh.ply").read_bytes() == (tmp_path / "py_mesh.ply").read_bytes(), "the saved PLY: node and python differ"
    assert (tmp_path / "out_trainer_tsdf.f32").read_bytes() == tT.tobytes(), "Trainer.fuseDepth tsdf: node and python differ"
    assert (tmp_path / "out_trainer_rgb.f32").read_bytes() == trgb.tobytes(), "Trainer.fuseDepth rgb: node and python differ"
