"""GPU: mesh connected components and small-component removal through the node host (bindings/napi/meshclean_run.js over the N-API addon) and the Python host
on the same inputs -- the cluster and star meshes with several selections and the two-sphere volume of tests/test_gpu_meshclean.py: SHA-256 digests of the
outputs, equal."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops

import meshclean_ref as M
from test_gpu_meshclean import _cluster_mesh, _volume_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _label_digests(r):
    return dict(count=r["count"], invalidFaces=r["invalidFaces"], **{k: _digest(r[k]) for k in ("faceComponent", "vertexComponent", "triangles", "vertices")})


def _mesh_digests(m):
    return {k: _digest(m[k]) for k in ("vertices", "faces", "vertexMap", "faceMap", "components", "colours", "keys") if m.get(k) is not None}


def test_node_mesh_components_equal_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cluster, lab = _cluster_mesh()
    star_faces, star_v, _ = M.shape("star-high-hub")
    cases = [("clusters", dict(vertices=cluster["vertices"], faces=cluster["faces"]),
              [dict(keepLargest=1), dict(keepLargest=7), dict(minTriangles=7), dict(minFraction=0.02), dict(keepLargest=0), dict()]),
             ("star", M.as_mesh(star_faces, star_v), [dict(keepLargest=1)])]
    want = dict(meshes={})
    meta = dict(meshes=[], volume=dict(origin=[float(x) for x in M.TS_ORIGIN], voxel_size=M.TS_VOXEL, dims=list(M.TS_DIMS), truncation=M.TS_TRUNC))
    for name, mesh, selections in cases:
        mesh["vertices"].tofile(str(tmp_path / f"{name}.vertices.f32"))
        mesh["faces"].tofile(str(tmp_path / f"{name}.faces.u32"))
        meta["meshes"].append(dict(name=name, selections=selections))
        want["meshes"][name] = dict(labels=_label_digests(ops.meshComponents(dev, mesh)),
                                    kept={str(i): _mesh_digests(ops.removeSmallComponents(dev, mesh, **sel)) for i, sel in enumerate(selections)})
    both, _, W, rgb = M.two_sphere_fields()
    for name, a in (("tsdf", both), ("weight", W), ("rgb", rgb)):
        np.ascontiguousarray(a, np.float32).tofile(str(tmp_path / f"volume.{name}.f32"))
    two = _volume_mesh(dev, both, W, rgb)
    want["spheres"] = dict(labels=_label_digests(ops.meshComponents(dev, two)), kept=_mesh_digests(ops.removeSmallComponents(dev, two, keepLargest=1)))
    assert want["spheres"]["labels"]["count"] == 2 and {"colours", "keys"} <= set(want["spheres"]["kept"])
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshclean_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHCLEAN_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["meshes"]:
        assert out["meshes"][name]["labels"] == want["meshes"][name]["labels"], name
        assert out["meshes"][name]["kept"] == want["meshes"][name]["kept"], (name, [k for k in want["meshes"][name]["kept"]
                                                                                     if out["meshes"][name]["kept"].get(k) != want["meshes"][name]["kept"][k]])
    assert out["spheres"] == want["spheres"], (out["spheres"], want["spheres"])
