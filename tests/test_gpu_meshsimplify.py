"""GPU: mesh simplification by vertex clustering on the device (csrc/meshsimplify.hip).  Every output byte equals the numpy
restatement (tests/meshsimplify_ref.py) on its crafted meshes -- empty inputs, the cell edges, non-finite coordinates, bad indices, rotations and duplicates,
the hot cell, the wave and block edges of the aggregation, random meshes, a face count of several scan blocks -- then capacity and state errors, recording,
repeats and reuse, the two-sphere TSDF volume, and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshclean_ref as M
import meshsimplify_ref as S
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
STATS = ("clusters", "invalid", "outside", "collapsed", "duplicate", "vertices", "faces")


def _assert_result(got, want, what, keys=S.OUTPUTS, rgb=False):
    for k in keys:
        w = want[k]
        if w is None:
            assert got[k] is None, f"{what}: {k}"
            continue
        if k == "colours" and rgb:
            w = np.ascontiguousarray(w[:, :3])
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
        assert_bits_equal(got[k], w, f"{what}: {k}")
    assert {k: got["stats"][k] for k in STATS} == {k: want["stats"][k] for k in STATS}, f"{what}: {got['stats']}"


def _upload(dev, m):
    V, F = m["vertices"].shape[0], m["faces"].shape[0]
    return dict(vertices=dev.bufferFrom(m["vertices"]), faces=dev.bufferFrom(m["faces"]), colours=None if m["colours"] is None else dev.bufferFrom(m["colours"]),
                V=V, F=F, origin=m["origin"], cell=m["cell"])


def _outputs(dev, nv, nf, V, colours=True):
    return dict(vertices=dev.createBuffer(12 * nv), faces=dev.createBuffer(12 * nf), colours=dev.createBuffer(4 * nv) if colours else None,
                keys=dev.createBuffer(8 * nv), faceMap=dev.createBuffer(4 * nf), vertexCluster=dev.createBuffer(4 * V))


def _count(simp, src):
    return simp.count(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], src["origin"], src["cell"])


def _emit(simp, src, outs, **kw):
    simp.emit(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], outs["vertices"], outs["faces"], outs["colours"], outs["keys"], outs["faceMap"],
              outs["vertexCluster"], **kw)


def _read(outs, nv, nf, V):
    return dict(vertices=outs["vertices"].read(np.float32, count=3 * nv).reshape(nv, 3), faces=outs["faces"].read(np.uint32, count=3 * nf).reshape(nf, 3),
                colours=None if outs["colours"] is None else outs["colours"].read(np.uint8, count=4 * nv).reshape(nv, 4), keys=outs["keys"].read(np.uint64, count=nv),
                faceMap=outs["faceMap"].read(np.uint32, count=nf), vertexCluster=outs["vertexCluster"].read(np.uint32, count=V))


def _simplify_with(dev, simp, m):
    """The result of ``m`` through ``simp``, every array read back (colours as rgba), with the count's statistics."""
    src = _upload(dev, m)
    nv, nf = _count(simp, src)
    outs = _outputs(dev, nv, nf, src["V"], src["colours"] is not None)
    _emit(simp, src, outs)
    got = _read(outs, nv, nf, src["V"])
    dev.synchronize()
    got["stats"] = simp.stats()
    return got


# ---------------------------------------------------------------- 1. the crafted meshes
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_device_simplification_equals_the_restatement(hip_device, name):
    dev = hip_device
    m, want = S.case(name), S.expected(name)
    simp = ops.MeshSimplifier(dev)
    try:
        got = _simplify_with(dev, simp, m)
    finally:
        simp.destroy()
    _assert_result(got, want, name)
    for k, n in S.EXPECT.get(name, {}).items():
        assert got["stats"][k] == n, f"{name}: {k}"
    _assert_result(ops.simplifyMesh(dev, m, m["cell"], m["origin"]), want, f"simplifyMesh: {name}", rgb=True)


def test_the_hot_cell_representative(hip_device):
    m = S.case("hot-cell")
    n = 30000
    got = ops.simplifyMesh(hip_device, m, m["cell"], m["origin"])
    hot = int(got["vertexCluster"][0])
    assert np.all(got["vertexCluster"][:n] == hot) and got["stats"]["clusters"] == 3
    t, c, _ = S.cells_of(m["vertices"][:n], m["origin"], m["cell"])
    q = ((t - c) * np.float32(65536.0)).astype(np.uint32).astype(np.int64)
    qm = (2 * q.sum(axis=0) + n) // (2 * n)
    cell = np.float32(m["cell"])
    want = m["origin"] + (c[0] + (qm.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -16)) * cell
    assert want.dtype == np.float32
    assert_bits_equal(got["vertices"][hot], want, "the hot cell's representative")
    col = m["colours"][:n].astype(np.int64)
    assert np.array_equal(got["colours"][hot], ((2 * col.sum(axis=0) + n) // (2 * n))[:3])


def test_origin_defaults_and_argument_errors(hip_device):
    dev = hip_device
    m = S.case("non-finite")
    finite = m["vertices"][np.all(np.isfinite(m["vertices"]), axis=1)]
    want = S.simplify(m["vertices"], m["faces"], m["colours"], finite.min(axis=0), 0.75)
    _assert_result(ops.simplifyMesh(dev, m, 0.75), want, "origin=None: the minimum of the finite vertices", rgb=True)
    rgb = dict(m, colours=np.ascontiguousarray(m["colours"][:, :3]))
    padded = S.simplify(m["vertices"], m["faces"], np.concatenate([rgb["colours"], np.full((9, 1), 255, np.uint8)], axis=1), m["origin"], m["cell"])
    _assert_result(ops.simplifyMesh(dev, rgb, m["cell"], m["origin"]), padded, "u8[V,3] colours", rgb=True)
    src = _upload(dev, m)
    with pytest.raises(ValueError):   # a device mesh has no default origin
        ops.simplifyMesh(dev, dict(vertices=src["vertices"], faces=src["faces"], colours=src["colours"]), 1.0)
    simp = ops.MeshSimplifier(dev)
    try:
        for cell in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(_lib.WdgsError) as e:
                simp.count(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], src["origin"], cell)
            assert e.value.code == _lib.WDGS_E_INVALID, cell
        for origin in ((0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0)):
            with pytest.raises(_lib.WdgsError) as e:
                simp.count(src["vertices"], src["V"], src["faces"], src["F"], src["colours"], origin, 1.0)
            assert e.value.code == _lib.WDGS_E_INVALID, origin
        for V, F in ((2 ** 31, 1), (1, 2 ** 31)):
            with pytest.raises(_lib.WdgsError) as e:
                simp.count(src["vertices"], V, src["faces"], F, src["colours"], src["origin"], 1.0)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.WdgsError):
            simp.count(None, 3, src["faces"], src["F"], None, src["origin"], 1.0)
    finally:
        simp.destroy()


# ---------------------------------------------------------------- 2. errors, recording, repeats
def test_capacity_state_and_recording(hip_device):
    dev = hip_device
    m, want = S.case("random"), S.expected("random")
    nv, nf, V = want["vertices"].shape[0], want["faces"].shape[0], m["vertices"].shape[0]
    src = _upload(dev, m)
    outs = _outputs(dev, nv, nf, V)
    simp = ops.MeshSimplifier(dev)
    try:
        with pytest.raises(_lib.StateError):
            simp.stats()
        with pytest.raises(_lib.StateError):   # no count precedes it
            _emit(simp, src, outs)
        assert _count(simp, src) == (nv, nf)
        for b in outs.values():
            b.write(np.full(b.size // 4, SENTINEL, np.uint32))
        for cv, cf in ((nv - 1, nf), (nv, nf - 1), (0, 0)):
            with pytest.raises(_lib.CapacityError):
                _emit(simp, src, outs, capacityVertices=cv, capacityFaces=cf)
        with pytest.raises(_lib.StateError):   # a count of other arguments
            simp.emit(src["vertices"], V, src["faces"], src["F"] - 1, src["colours"], outs["vertices"], outs["faces"], outs["colours"], outs["keys"])
        other = dev.bufferFrom(m["vertices"])
        with pytest.raises(_lib.StateError):
            simp.emit(other, V, src["faces"], src["F"], src["colours"], outs["vertices"], outs["faces"], outs["colours"], outs["keys"])
        dev.synchronize()
        for k, b in outs.items():
            assert np.all(b.read(np.uint32) == SENTINEL), f"a refused emit wrote {k}"
        _emit(simp, src, outs)
        eager = dict(_read(outs, nv, nf, V), stats=simp.stats())
        _assert_result(eager, want, "emit after the refusals")
        # the emit waits for nothing and records
        for b in outs.values():
            b.clear()
        with dev.createCommandEncoder("simplify emit", record=True) as enc:
            _emit(simp, src, outs)
            cmd = enc.finish()
        assert np.all(outs["faces"].read(np.uint32) == 0), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        _assert_result(dict(_read(outs, nv, nf, V), stats=simp.stats()), eager, "a recorded emit, replayed")
        cmd.destroy()
        # the optional outputs left out
        for b in outs.values():
            b.clear()
        simp.emit(src["vertices"], V, src["faces"], src["F"], src["colours"], outs["vertices"], outs["faces"], outs["colours"])
        _assert_result(dict(_read(outs, nv, nf, V), stats=simp.stats()), eager, "emit without keys and maps", ("vertices", "faces", "colours"))
        assert np.all(outs["keys"].read(np.uint32) == 0) and np.all(outs["faceMap"].read(np.uint32) == 0)
        with pytest.raises(_lib.StateError):   # the count waits for its totals
            with dev.createCommandEncoder("doomed", record=True):
                _count(simp, src)
        dev.synchronize()
        with pytest.raises(_lib.StateError):   # a refused count leaves nothing to emit
            _emit(simp, src, outs)
    finally:
        simp.destroy()
        simp.destroy()   # idempotent


def test_two_runs_agree_and_one_simplifier_takes_meshes_of_any_size(hip_device):
    dev = hip_device
    m = S.case("many-faces")
    a, b = ops.simplifyMesh(dev, m, m["cell"], m["origin"]), ops.simplifyMesh(dev, m, m["cell"], m["origin"])
    _assert_result(b, a, "a second run")
    simp = ops.MeshSimplifier(dev)
    try:
        for name in ("three-cells", "random", "many-faces", "no-faces", "row-4097", "nothing", "hot-cell", "no-vertices", "random-no-colours", "rotations"):
            _assert_result(_simplify_with(dev, simp, S.case(name)), S.expected(name), f"reused simplifier: {name}")
    finally:
        simp.destroy()


def test_one_simplification_is_three_sorts_launch_for_launch(hip_device):
    """The launch sequence of one count + emit, pinned: three stable u64 sorts (csrc/keysort.hip) -- the six sort labels three times, the two per-pass
    ones twenty-four -- every simplify_* kernel once, and the library scan's three kernels 29 times each: three times eight digit tables and head
    flags, then the cluster and face flags.  The scan_* literals are what the library gave on this mesh before the sort became one object; the others
    follow from the code."""
    dev = hip_device
    m = S.case("random")
    assert (m["vertices"].shape[0], m["faces"].shape[0]) == (20481, 40000)
    src = _upload(dev, m)
    simp = ops.MeshSimplifier(dev)
    try:
        outs = _outputs(dev, src["V"], src["F"], src["V"])
        dev.synchronize()
        dev.setProfiling(True)
        dev.kernelTimes(reset=True)
        _count(simp, src)
        _emit(simp, src, outs)
        dev.synchronize()
        dev.setProfiling(False)
        times = dev.kernelTimes(reset=True)
    finally:
        dev.setProfiling(False)
        simp.destroy()
    launches = {k: v[0] for k, v in times.items()}
    print("launches:", sorted(launches.items()))
    assert {k: n for k, n in launches.items() if k.startswith("weld_")} == dict(weld_key_bits=3, weld_plan=3, weld_histogram=24, weld_scatter=24, weld_heads=3,
                                                                                  weld_emit=3), launches
    simplify = ("cell_keys", "accumulate", "finalize", "face_keys", "fold", "face_keys2", "mark", "emit_vertices", "emit_faces")
    assert {k: n for k, n in launches.items() if k.startswith("simplify_")} == {f"simplify_{k}": 1 for k in simplify}, launches
    assert {k: n for k, n in launches.items() if k.startswith("scan_")} == dict(scan_reduce=29, scan_block_sums=29, scan_downsweep=29), launches


# ---------------------------------------------------------------- 3. two spheres in a TSDF volume
def _rgba(mesh):
    return None if mesh["colours"] is None else np.concatenate([mesh["colours"], np.full((mesh["colours"].shape[0], 1), 255, np.uint8)], axis=1)


def test_two_sphere_volume_simplifies_to_the_restatement(hip_device):
    dev = hip_device
    both, _, wt, rgb = M.two_sphere_fields()
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    welded, simplified = {}, {}
    cell = 2.0 * M.TS_VOXEL
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        host = vol.extractMesh()
        want = S.simplify(host["vertices"], host["faces"], _rgba(host), M.TS_ORIGIN, cell)
        assert 0 < want["faces"].shape[0] < host["faces"].shape[0] and 0 < want["vertices"].shape[0] < host["vertices"].shape[0]
        mine = ops.simplifyMesh(dev, host, cell, origin=M.TS_ORIGIN)
        _assert_result(mine, want, "simplifyMesh of extractMesh()", rgb=True)
        _assert_result(vol.extractMesh(weld="device", simplify=cell), mine, "extractMesh(weld='device', simplify=)")
        _assert_result(vol.extractMesh(simplify=cell), mine, "extractMesh(simplify=)")
        again = vol.extractMesh()
        for k in ("vertices", "faces", "colours", "keys"):
            assert_bits_equal(again[k], host[k], f"simplify=None: {k}")
        assert set(again) == {"vertices", "faces", "colours", "keys"}
        # asBuffers: device buffers of exactly the result's sizes, which the rest of the chain accepts
        tri = vol.extractTriangleBuffers()
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        ops.destroyBuffers(tri)
        simplified = ops.simplifyMesh(dev, welded, cell, origin=M.TS_ORIGIN, asBuffers=True)
        nv, nf = simplified["numVertices"], simplified["numFaces"]
        assert (nv, nf) == (want["vertices"].shape[0], want["faces"].shape[0])
        assert [simplified[k].size for k in ("vertices", "faces", "colours", "keys", "faceMap", "vertexCluster")] == [12 * nv, 12 * nf, 4 * nv, 8 * nv, 4 * nf,
                                                                                                                      4 * welded["numVertices"]]
        assert_bits_equal(simplified["vertices"].read(np.float32).reshape(nv, 3), want["vertices"], "asBuffers: vertices")
        assert_bits_equal(simplified["faces"].read(np.uint32).reshape(nf, 3), want["faces"], "asBuffers: faces")
        on_device = dict(vertices=simplified["vertices"], faces=simplified["faces"])
        lab = ops.meshComponents(dev, on_device)
        assert lab["count"] == 2 and lab["invalidFaces"] == 0
        a, b = ops.sampleMesh(dev, on_device, 50.0, 3), ops.sampleMesh(dev, mine, 50.0, 3)
        assert a["points"].shape[0] > 0
        assert_bits_equal(a["points"], b["points"], "asBuffers into sampleMesh")
        twice = ops.simplifyMesh(dev, simplified, 2.0 * cell, origin=M.TS_ORIGIN)
        _assert_result(twice, ops.simplifyMesh(dev, mine, 2.0 * cell, origin=M.TS_ORIGIN), "asBuffers into simplifyMesh")
    finally:
        ops.destroyBuffers(welded)
        ops.destroyBuffers(simplified)
        vol.destroy()


# ---------------------------------------------------------------- 4. the Trainer surface
def test_trainer_extract_mesh_simplifies_last(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    cell = 2.0 * voxel
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    try:
        for _ in range(4):
            t.step()
        t.drain()
        iteration, rng_state = t.iteration, t._rng.getstate()
        t.fuseDepth(vol)
        parent = ops.weldTriangles(vol.extractTriangles(1.0))
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == {"vertices", "faces", "colours", "keys"} and raw["faces"].shape[0] > 0
        for k in raw:
            assert_bits_equal(raw[k], parent[k], f"simplify=None still equals the parent's output: {k}")
        want = ops.simplifyMesh(dev, raw, cell, origin=vol.origin)
        assert 0 < want["faces"].shape[0] < raw["faces"].shape[0]
        for weld in ("host", "device"):
            got = t.extractMesh(lo, hi, voxel, weld=weld, simplify=cell)
            assert list(got) == list(want)
            _assert_result(got, want, f"extractMesh(weld={weld!r}, simplify=)")
        largest = t.extractMesh(lo, hi, voxel, keepLargest=1)
        assert largest["faces"].shape[0] < raw["faces"].shape[0], "the scene's level set has floaters"
        want1 = ops.simplifyMesh(dev, largest, cell, origin=vol.origin)
        for weld in ("host", "device"):
            _assert_result(t.extractMesh(lo, hi, voxel, keepLargest=1, weld=weld, simplify=cell), want1, f"extractMesh(keepLargest=1, weld={weld!r}, simplify=)")
        assert want1["faces"].shape[0] < want["faces"].shape[0]
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        plain = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1)
        for weld in ("host", "device"):
            out = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1, weld=weld, simplify=cell)
            assert (out["vertices"], out["faces"]) == (want1["vertices"].shape[0], want1["faces"].shape[0])
            for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore"):
                assert np.isfinite(out[k]), f"evaluateGeometry(simplify=): {k} = {out[k]}"
            print(f"evaluateGeometry weld={weld}: simplified " + ", ".join(f"{k}={out[k]:.6g}" for k in ("accuracy", "completeness", "chamfer", "fscore", "faces"))
                  + " | unsimplified " + ", ".join(f"{k}={plain[k]:.6g}" for k in ("accuracy", "completeness", "chamfer", "fscore", "faces")))
        assert t.iteration == iteration and t._rng.getstate() == rng_state
    finally:
        vol.destroy()
        t.destroy()
