"""GPU: the k-nearest query and the neighbour-based scales through the node host (bindings/napi/knn_run.js over the N-API addon) and the Python host on the
same inputs -- the random case for every k and cutoff and the loaded 600-point cloud of tests/test_gpu_knn.py: SHA-256 digests of the outputs, equal."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops

import test_knn_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_node_knn_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    pts, qs = R.random_case()
    data = R.scales_case()
    cell, small_cutoff = 0.06, 1.5
    want = dict(knn={}, scales={})
    index = ops.PointIndex(dev, pts, cellSize=cell)
    try:
        for c, cutoff in enumerate(R.RANDOM_CUTOFFS):
            for k in R.RANDOM_KS:
                r = index.kNearest(qs, k, cutoff)
                want["knn"][f"{c}/{k}"] = dict(d2=_digest(r["d2"]), index=_digest(r["index"]))
        r = index.kNearest(pts, 3, R.RANDOM_CUTOFFS[0], excludeSelf=True)
        want["knn"]["self"] = dict(d2=_digest(r["d2"]), index=_digest(r["index"]))
        bounds = index.bounds()
    finally:
        index.destroy()
    for name, max_distance in (("default", None), ("small", small_cutoff)):
        pc = ops.createPointCloud(dev, data.gaussians, data.sh, data.sh_deg)
        out = ops.initScalesFromNeighbours(dev, pc, k=3, maxDistance=max_distance)
        want["scales"][name] = dict(gaussians=_digest(pc.gaussian_3d_buffer.read(np.uint32, count=6 * data.num_points)),
                                    sh=_digest(pc.sh_buffer.read(np.uint32, count=24 * data.num_points)), meanD2=_digest(out["meanD2"]), found=_digest(out["found"]))
    assert want["scales"]["default"]["gaussians"] != want["scales"]["small"]["gaussians"] != _digest(data.gaussians)
    pts.tofile(str(tmp_path / "points.f32"))
    qs.tofile(str(tmp_path / "queries.f32"))
    data.gaussians.tofile(str(tmp_path / "gaussians.u32"))
    data.sh.tofile(str(tmp_path / "sh.u32"))
    (tmp_path / "meta.json").write_text(json.dumps(dict(cell_size=cell, cutoffs=list(R.RANDOM_CUTOFFS), ks=list(R.RANDOM_KS), small_cutoff=small_cutoff,
                                                        num_points=data.num_points)))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "knn_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "KNN_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    assert out["knn"] == want["knn"], [key for key in want["knn"] if out["knn"].get(key) != want["knn"][key]]
    assert out["scales"] == want["scales"], (out["scales"], want["scales"])
    assert out["bounds"] == dict(lo=[float(x) for x in bounds["lo"]], hi=[float(x) for x in bounds["hi"]])
