"""GPU: mesh adjacency, Taubin smoothing and vertex normals through the node host (bindings/napi/meshsmooth_run.js over the N-API addon) and the Python host
on the same inputs -- the crafted meshes of tests/meshsmooth_ref.py and the two-sphere volume: SHA-256 digests of the outputs, equal, and equal to the
restatement's."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import loaders, ops

import meshclean_ref as M
import meshsmooth_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMPLIFY_STATS = ("clusters", "invalid", "outside", "collapsed", "duplicate", "vertices", "faces")


def mesh_digest(mesh):
    """sha256 over a mesh's arrays in a fixed order, then its statistics (bindings/napi/meshsmooth_run.js: meshDigest)."""
    h = hashlib.sha256()
    for k in ("vertices", "faces", "colours", "keys", "faceMap", "vertexCluster", "normals"):
        if mesh.get(k) is not None:
            h.update(np.ascontiguousarray(mesh[k]).tobytes())
    stats = mesh.get("stats") or {}
    h.update(np.array([stats[k] for k in (SIMPLIFY_STATS if "clusters" in stats else R.STATS if stats else ())], np.uint32).tobytes())
    return h.hexdigest()


def test_node_smoothing_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cell, smooth = 2.0 * M.TS_VOXEL, 3
    meta = dict(meshes=[], volume=dict(origin=[float(x) for x in M.TS_ORIGIN], voxel_size=M.TS_VOXEL, dims=list(M.TS_DIMS), truncation=M.TS_TRUNC, cell=cell,
                                       smooth=smooth))
    want = dict(meshes={})
    for name in sorted(R.CASES):
        m, e = R.case(name), R.expected(name)
        m["vertices"].tofile(str(tmp_path / f"{name}.vertices.f32"))
        m["faces"].tofile(str(tmp_path / f"{name}.faces.u32"))
        meta["meshes"].append(dict(name=name, **m["smoothing"]))
        want["meshes"][name] = dict(device=R.digest(e), host=R.digest(e), stats=e["stats"])
    both, _, wt, rgb = M.two_sphere_fields()
    for name, a in (("tsdf", both), ("weight", wt), ("rgb", rgb)):
        np.ascontiguousarray(a, np.float32).tofile(str(tmp_path / f"volume.{name}.f32"))
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        plain = vol.extractMesh()
        smoothed = vol.extractMesh(weld="device", smooth=smooth, normals=True)
        simplified = vol.extractMesh(weld="device", smooth=smooth, simplify=cell, normals=True)
    finally:
        vol.destroy()
    assert smoothed["vertices"].tobytes() == R.smooth(plain["vertices"], plain["faces"], smooth).tobytes()
    d, ds = mesh_digest(smoothed), mesh_digest(simplified)
    want["spheres"] = dict(plain=mesh_digest(plain), defaults=mesh_digest(plain), host=d, device=d, ofMesh=d, simplifiedHost=ds, simplifiedDevice=ds,
                           ply=hashlib.sha256(loaders.meshPLYBytes(smoothed)).hexdigest(), plyPlain=hashlib.sha256(loaders.meshPLYBytes(plain)).hexdigest())
    assert len({d, ds, want["spheres"]["plain"]}) == 3
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshsmooth_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHSMOOTH_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["meshes"]:
        assert out["meshes"][name] == want["meshes"][name], (name, out["meshes"][name], want["meshes"][name])
    assert out["spheres"] == want["spheres"], (out["spheres"], want["spheres"])
