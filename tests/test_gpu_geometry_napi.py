"""GPU: the mesh accuracy metrics through the node host (bindings/napi/geometry_run.js over the N-API addon) and the Python host on the same inputs: the
samples, the d2 and index arrays, the three sums, the metrics, the points PLY and Trainer.evaluateGeometry's numbers, byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import loaders, ops, synth
from webdgs_amd.trainer import Trainer

import geometry_ref as G
import harness
import test_geometry_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _jsonable(d):
    return {k: ("nan" if isinstance(v, float) and np.isnan(v) else v) for k, v in d.items()}


def test_node_geometry_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    density, seed, cutoff, threshold, cell = 700.0, 6, 0.09, 0.05, 0.04
    v, f = G.square_mesh(12, size=3.0)
    v[:, 2] += (0.37 * v[:, 0] - 0.21 * v[:, 1]).astype(np.float32)
    pts, qs = R.random_cloud(3000, 21), R.random_cloud(2000, 22)
    samples = ops.sampleMesh(dev, dict(vertices=v, faces=f), density, seed)
    index = ops.PointIndex(dev, pts, cellSize=cell)
    try:
        near = index.nearest(qs, cutoff)
        info = index.info()
    finally:
        index.destroy()
    stats = ops.pointDistanceStats(dev, near["d2"], cutoff, threshold)
    metrics = ops.geometryMetrics(dev, qs, pts, cutoff, threshold)
    loaders.savePointsPLY(str(tmp_path / "py_samples.ply"), samples["points"])
    # the Python Trainer's evaluateGeometry before any step (blank images: never looked at), against a plane inside the scene's box
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh = synth.make_gaussians(cfg)
    cams = synth.circle_cameras(cfg, 4)
    lo, hi, voxel = [-2.01, -1.52, 2.03], [2.0, 1.5, 9.0], 0.11
    rv = np.array([[lo[0], lo[1], 5], [hi[0], lo[1], 5], [hi[0], hi[1], 5], [lo[0], hi[1], 5]], np.float32)
    reference = G.sample_mesh(rv, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 100.0, 1)["points"]
    loaders.savePointsPLY(str(tmp_path / "reference.ply"), reference)
    train_views, fuse_order = [0, 1, 3], [2, 0]
    n = cfg.width * cfg.height
    t = Trainer(dev, seed=5)
    try:
        t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
        t.setDataset([dict(camera=cams[i], width=cfg.width, height=cfg.height) for i in train_views],
                     [dict(texture=dev.bufferFrom(np.zeros(4 * n, np.uint8)), width=cfg.width, height=cfg.height) for _ in train_views])
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.start()
        evaluated = t.evaluateGeometry(str(tmp_path / "reference.ply"), lo, hi, voxel, maxDistance=8.0, threshold=0.5, seed=seed, viewIds=fuse_order)
    finally:
        t.destroy()
    assert evaluated["samples"] > 0 and np.isfinite(evaluated["chamfer"])
    del evaluated["ms"]
    v.tofile(str(tmp_path / "mesh_vertices.f32"))
    f.tofile(str(tmp_path / "mesh_faces.u32"))
    pts.tofile(str(tmp_path / "points.f32"))
    qs.tofile(str(tmp_path / "queries.f32"))
    (tmp_path / "meta.json").write_text(json.dumps(dict(config=dict(config_id=cfg.config_id, num_points=cfg.num_points, width=cfg.width, height=cfg.height,
                                                                    sh_deg=cfg.sh_deg, fy=cfg.fy, s0=cfg.s0, name=cfg.name), cameras=4,
                                                        density=density, seed=seed, cutoff=cutoff, threshold=threshold, cell_size=cell, lo=lo, hi=hi, voxel_size=voxel,
                                                        eval_max_distance=8.0, eval_threshold=0.5, train_views=train_views, fuse_order=fuse_order)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "geometry_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GEOMETRY_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    assert out["samples"] == samples["points"].shape[0] > 0
    assert (tmp_path / "out_samples.f32").read_bytes() == samples["points"].tobytes(), "samples: node and python differ"
    assert (tmp_path / "out_face.u32").read_bytes() == samples["face"].tobytes(), "sample faces: node and python differ"
    assert (tmp_path / "out_samples.ply").read_bytes() == (tmp_path / "py_samples.ply").read_bytes(), "the points PLY: node and python differ"
    assert (tmp_path / "out_d2.f32").read_bytes() == near["d2"].tobytes(), "d2: node and python differ"
    assert (tmp_path / "out_index.u32").read_bytes() == near["index"].tobytes(), "index: node and python differ"
    assert out["info"]["dims"] == list(info["dims"]) and out["info"]["indexed"] == info["indexed"] and out["info"]["cellSize"] == info["cellSize"]
    assert out["stats"] == _jsonable(stats), (out["stats"], stats)
    assert out["metrics"] == _jsonable(metrics), (out["metrics"], metrics)
    assert out["evaluated"] == _jsonable(evaluated), (out["evaluated"], evaluated)
