"""GPU: welding on the device through the node host (bindings/napi/meshweld_run.js over the N-API addon) and the Python host on the same inputs -- the
crafted soups of tests/meshweld_ref.py and the two-sphere volume of tests/test_gpu_meshclean.py: SHA-256 digests of the outputs, equal."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops

import meshclean_ref as M
import meshweld_ref as W
from test_gpu_meshclean import _volume_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mesh_digests(m):
    return {k: _digest(m[k]) for k in ("vertices", "faces", "vertexMap", "faceMap", "components", "colours", "keys") if m.get(k) is not None}


def test_node_device_weld_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    want = dict(soups={})
    meta = dict(soups=sorted(W.CASES), volume=dict(origin=[float(x) for x in M.TS_ORIGIN], voxel_size=M.TS_VOXEL, dims=list(M.TS_DIMS), truncation=M.TS_TRUNC))
    for name in meta["soups"]:
        tri = W.case(name)
        for key, ext in (("keys", "keys.u64"), ("positions", "positions.f32"), ("colours", "colours.u8")):
            tri[key].tofile(str(tmp_path / f"{name}.{ext}"))
        mesh = ops.weldTrianglesDevice(dev, tri)
        want["soups"][name] = dict(_mesh_digests(mesh), numVertices=int(mesh["keys"].shape[0]))
        if name in W.PASSES_RUN:
            want["soups"][name]["passesRun"] = W.PASSES_RUN[name]
    both, _, wt, rgb = M.two_sphere_fields()
    for name, a in (("tsdf", both), ("weight", wt), ("rgb", rgb)):
        np.ascontiguousarray(a, np.float32).tofile(str(tmp_path / f"volume.{name}.f32"))
    two = _volume_mesh(dev, both, wt, rgb)
    want["spheres"] = dict(host=_mesh_digests(two), device=_mesh_digests(two), kept=_mesh_digests(ops.removeSmallComponents(dev, dict(vertices=two["vertices"], faces=two["faces"]), keepLargest=1)))
    assert {"colours", "keys"} <= set(want["spheres"]["host"])
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshweld_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHWELD_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in meta["soups"]:
        got = out["soups"][name]
        if name not in W.PASSES_RUN:
            got.pop("passesRun")
        assert got == want["soups"][name], (name, got, want["soups"][name])
    assert out["spheres"] == want["spheres"], (out["spheres"], want["spheres"])
