"""GPU: simplification by vertex clustering through the node host (bindings/napi/meshsimplify_run.js over the N-API addon) and the Python host on the same
inputs -- the crafted meshes of tests/meshsimplify_ref.py and the two-sphere volume: SHA-256 digests of the outputs, equal, and equal to the restatement's."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webdgs_amd import ops

import meshclean_ref as M
import meshsimplify_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_simplification_equals_the_python_hosts(hip_device, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "bindings", "napi", "webdgs_napi.node")
    if not node or not os.path.exists(addon):
        pytest.skip("node or the N-API addon is not available")
    dev = hip_device
    cell = 2.0 * M.TS_VOXEL
    meta = dict(meshes=[], volume=dict(origin=[float(x) for x in M.TS_ORIGIN], voxel_size=M.TS_VOXEL, dims=list(M.TS_DIMS), truncation=M.TS_TRUNC, cell=cell))
    want = dict(meshes={})
    for name in sorted(S.CASES):
        m = S.case(name)
        for key, ext in (("vertices", "vertices.f32"), ("faces", "faces.u32"), ("colours", "colours.u8")):
            if m[key] is not None:
                m[key].tofile(str(tmp_path / f"{name}.{ext}"))
        meta["meshes"].append(dict(name=name, origin=[float(x) for x in m["origin"]], cell=m["cell"], colours=m["colours"] is not None))
        host = ops.simplifyMesh(dev, m, m["cell"], m["origin"])
        want["meshes"][name] = dict(host=S.digest(host), device=S.digest(S.expected(name)), stats=host["stats"])
        assert host["stats"] == S.expected(name)["stats"]
    both, _, wt, rgb = M.two_sphere_fields()
    for name, a in (("tsdf", both), ("weight", wt), ("rgb", rgb)):
        np.ascontiguousarray(a, np.float32).tofile(str(tmp_path / f"volume.{name}.f32"))
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        plain = vol.extractMesh()
        simplified = vol.extractMesh(weld="device", simplify=cell)
    finally:
        vol.destroy()
    d = S.digest(simplified)
    samples = ops.sampleMesh(dev, simplified, 50.0, 3)
    want["spheres"] = dict(host=d, device=d, ofMesh=d, plainFaces=int(plain["faces"].shape[0]), faces=int(simplified["faces"].shape[0]),
                           components=int(ops.meshComponents(dev, simplified)["count"]), samples=hashlib.sha256(samples["points"].tobytes()).hexdigest())
    assert want["spheres"]["faces"] < want["spheres"]["plainFaces"] and want["spheres"]["components"] == 2
    (tmp_path / "meta.json").write_text(json.dumps(meta))
    r = subprocess.run([node, os.path.join(ROOT, "bindings", "napi", "meshsimplify_run.js"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MESHSIMPLIFY_RUN_OK" in r.stdout, f"exit code {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads((tmp_path / "out.json").read_text())
    assert out["errors"] == [], out["errors"]
    for name in want["meshes"]:
        assert out["meshes"][name] == want["meshes"][name], (name, out["meshes"][name], want["meshes"][name])
    assert out["spheres"] == want["spheres"], (out["spheres"], want["spheres"])
