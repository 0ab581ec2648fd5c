"""GPU: mesh connected components and small-component removal (csrc/meshclean.hip) against the restatement (tests/meshclean_ref.py).
Every comparison is byte equality: the labelling on clusters, chains, stars, singletons, late bridges and the edge cases, the compaction for every rule of
the selection, capacity and state errors, determinism and device-resident input, two spheres in a TSDF volume, and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshclean_ref as M
import tsdf64 as t64
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views
from test_gpu_geometry import _same_metrics

pytestmark = pytest.mark.gpu

LABEL_KEYS = ("faceComponent", "vertexComponent", "triangles", "vertices")
MESH_KEYS = ("vertices", "faces", "vertexMap", "faceMap", "components")


def _assert_labels(got, want, what):
    assert (got["count"], got["invalidFaces"]) == (want["count"], want["invalidFaces"]), f"{what}: C and invalid faces {got['count']}, {got['invalidFaces']}"
    for k in LABEL_KEYS:
        assert got[k].dtype == np.uint32
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


def _assert_mesh(got, want, what, keys=MESH_KEYS):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, f"{what}: {k}"
            continue
        assert got[k].dtype == want[k].dtype, f"{what}: {k} is {got[k].dtype}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


def _cluster_mesh():
    faces, V, lab = M.shape("clusters")
    mesh = M.as_mesh(faces, V)
    mesh["keys"] = np.arange(V, dtype=np.uint64) * np.uint64(7) + np.uint64(2 ** 40)
    mesh["colours"] = (np.arange(3 * V) % 251).astype(np.uint8).reshape(V, 3)
    return mesh, lab


# ---------------------------------------------------------------- 1. the labelling
@pytest.mark.parametrize("name", sorted(M.SHAPES))
def test_labelling_equals_the_restatement(hip_device, name):
    faces, V, want = M.shape(name)
    got = ops.meshComponents(hip_device, M.as_mesh(faces, V))
    _assert_labels(got, want, name)


def test_labelling_is_deterministic_and_takes_device_meshes(hip_device):
    dev = hip_device
    faces, V, want = M.shape("clusters")
    mesh = M.as_mesh(faces, V)
    a, b = ops.meshComponents(dev, mesh), ops.meshComponents(dev, mesh)
    _assert_labels(b, a, "a second call")
    resident = dict(vertices=dev.bufferFrom(mesh["vertices"]), faces=dev.bufferFrom(mesh["faces"]))
    _assert_labels(ops.meshComponents(dev, resident), a, "a device-resident mesh")
    for kw in (dict(keepLargest=2), dict()):
        _assert_mesh(ops.removeSmallComponents(dev, resident, **kw), ops.removeSmallComponents(dev, mesh, **kw), f"a device-resident mesh, {kw}")
    # one object, meshes of different sizes one after the other: the arrays grow and nothing of the earlier mesh shows
    comp = ops.MeshComponents(dev)
    try:
        for name in ("one-face", "star-high-hub", "clusters", "no-faces", "singletons"):
            f, v, w = M.shape(name)
            buf = dev.bufferFrom(f)
            comp.label(buf, f.shape[0], v)
            _assert_labels(comp.read(), w, f"reused object: {name}")
    finally:
        comp.destroy()


# ---------------------------------------------------------------- 2. selection and compaction
def test_compaction_equals_the_restatement_for_every_rule(hip_device):
    dev = hip_device
    mesh, lab = _cluster_mesh()
    t = lab["triangles"].astype(np.int64)
    C = lab["count"]
    ranking = sorted(range(C), key=lambda c: (-t[c], c))
    # a cut between two components of equal size: the lower number stays
    cut = next(r for r in range(1, C) if t[ranking[r - 1]] == t[ranking[r]] and t[ranking[r]] > 1)
    shared = int(t[ranking[cut]])
    assert np.sum(t == shared) >= 2
    fraction = float(t[ranking[3]]) / float(t.max())
    rules = [dict(keepLargest=1), dict(keepLargest=2), dict(keepLargest=C), dict(keepLargest=C + 5), dict(keepLargest=0), dict(minTriangles=shared),
             dict(keepLargest=cut), dict(minFraction=fraction), dict(minFraction=0.5), dict(keepLargest=40, minTriangles=3, minFraction=0.01), dict()]
    for kw in rules:
        keep = M.select(lab["triangles"], **kw)
        assert_bits_equal(ops.selectComponents(lab["triangles"], **kw), keep, f"selectComponents {kw}")
        got, want = ops.removeSmallComponents(dev, mesh, **kw), M.remove_small(mesh, **kw)
        _assert_mesh(got, want, f"removeSmallComponents {kw}", MESH_KEYS + ("colours", "keys"))
        assert got["faces"].shape[0] == int(t[keep].sum())
        again = ops.removeSmallComponents(dev, got, **kw)
        _assert_mesh(again, got, f"compacting twice {kw}", ("vertices", "faces", "components", "colours", "keys"))
        assert np.array_equal(again["vertexMap"], np.arange(got["vertices"].shape[0])) and np.array_equal(again["faceMap"], np.arange(got["faces"].shape[0]))
    keep = M.select(lab["triangles"], minTriangles=shared)
    assert keep[t == shared].all() and not keep[t < shared].any()
    keep = M.select(lab["triangles"], keepLargest=cut)
    assert keep[ranking[cut - 1]] and not keep[ranking[cut]] and ranking[cut - 1] < ranking[cut]
    assert ops.removeSmallComponents(dev, mesh, keepLargest=0)["faces"].shape == (0, 3)
    # keeping everything: the input's faces without the invalid ones, renumbered
    everything = ops.removeSmallComponents(dev, mesh)
    valid = lab["faceComponent"] != M.NONE
    assert_bits_equal(everything["faceMap"], np.flatnonzero(valid).astype(np.uint32), "kept everything: the valid faces")
    assert_bits_equal(everything["vertexMap"][everything["faces"]], mesh["faces"][valid], "kept everything: the same triangles")
    assert everything["vertices"].shape[0] == int(np.sum(lab["vertexComponent"] != M.NONE))


def test_empty_meshes_compact_to_empty_meshes(hip_device):
    for name in ("no-faces", "no-vertices", "only-invalid", "one-face"):
        faces, V, _ = M.shape(name)
        mesh = M.as_mesh(faces, V)
        for kw in (dict(), dict(keepLargest=1), dict(keepLargest=0)):
            _assert_mesh(ops.removeSmallComponents(hip_device, mesh, **kw), M.remove_small(mesh, **kw), f"{name} {kw}")


def test_capacity_state_and_argument_errors(hip_device):
    dev = hip_device
    mesh, lab = _cluster_mesh()
    keep = M.select(lab["triangles"], keepLargest=3)
    want = M.compact(mesh, lab, keep)
    kv, kf = want["vertices"].shape[0], want["faces"].shape[0]
    vbuf, fbuf = dev.bufferFrom(mesh["vertices"]), dev.bufferFrom(mesh["faces"])
    comp = ops.MeshComponents(dev)
    try:
        with pytest.raises(_lib.StateError):
            comp.read()
        with pytest.raises(_lib.StateError):
            comp.select(keep)
        assert comp.label(fbuf, mesh["faces"].shape[0], mesh["vertices"].shape[0]) == lab["count"]
        outs = [dev.createBuffer(n) for n in (12 * kv, 12 * kf, 4 * kv, 4 * kf)]
        with pytest.raises(_lib.StateError):
            comp.compact(vbuf, *outs)
        with pytest.raises(_lib.WdgsError):
            comp.select(keep[:-1])
        assert comp.select(keep) == (kv, kf)
        pattern = np.full(3 * max(kv, kf), 0xA5A5A5A5, np.uint32)
        for b in outs:
            b.write(pattern[: b.size // 4])
        for cv, cf in ((kv - 1, kf), (kv, kf - 1), (0, 0)):
            with pytest.raises(_lib.CapacityError):
                comp.compact(vbuf, *outs, capacityVertices=cv, capacityFaces=cf)
        dev.synchronize()
        for b in outs:
            assert np.all(b.read(np.uint32) == 0xA5A5A5A5), "a refused compaction wrote something"
        comp.compact(vbuf, *outs)
        assert_bits_equal(outs[0].read(np.float32).reshape(kv, 3), want["vertices"], "compact: vertices")
        assert_bits_equal(outs[1].read(np.uint32).reshape(kf, 3), want["faces"], "compact: faces")
        assert_bits_equal(outs[2].read(np.uint32), want["vertexMap"], "compact: vertexMap")
        assert_bits_equal(outs[3].read(np.uint32), want["faceMap"], "compact: faceMap")
        # without positions and maps; a second selection on the same labelling
        outs[1].clear()
        comp.compact(None, None, outs[1])
        assert_bits_equal(outs[1].read(np.uint32).reshape(kf, 3), want["faces"], "compact without positions: faces")
        assert comp.select(np.ones(lab["count"], bool)) == (int(lab["vertices"].sum()), int(lab["triangles"].sum()))
        with pytest.raises(_lib.CapacityError):
            comp.compact(vbuf, *outs)
        with pytest.raises(_lib.WdgsError):
            comp.label(None, 3, 10)
        with pytest.raises(_lib.WdgsError):
            comp.label(fbuf, 2 ** 31, 10)
        with pytest.raises(_lib.WdgsError):
            comp.label(fbuf, 10, 2 ** 31)
        with pytest.raises(_lib.StateError):   # a refused labelling leaves nothing to read
            comp.read()
        with pytest.raises(_lib.StateError):   # the labelling waits for C
            with dev.createCommandEncoder("doomed", record=True):
                comp.label(fbuf, mesh["faces"].shape[0], mesh["vertices"].shape[0])
        dev.synchronize()
        # the compaction waits for nothing and records
        comp.label(fbuf, mesh["faces"].shape[0], mesh["vertices"].shape[0])
        assert comp.select(keep) == (kv, kf)
        for b in outs:
            b.clear()
        with dev.createCommandEncoder("compact", record=True) as enc:
            comp.compact(vbuf, *outs)
            cmd = enc.finish()
        assert np.all(outs[1].read(np.uint32) == 0), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        assert_bits_equal(outs[1].read(np.uint32).reshape(kf, 3), want["faces"], "recorded compact: faces")
        assert_bits_equal(outs[2].read(np.uint32), want["vertexMap"], "recorded compact: vertexMap")
        cmd.destroy()
    finally:
        comp.destroy()
        comp.destroy()   # idempotent
    with pytest.raises(ValueError):
        ops.selectComponents(lab["triangles"], keepLargest=-1)


# ---------------------------------------------------------------- 3. two spheres in a TSDF volume
def _volume_mesh(dev, T, W, rgb):
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(T, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(W, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        return vol.extractMesh()
    finally:
        vol.destroy()


def test_two_spheres_keep_largest_is_the_mesh_of_the_larger_sphere_alone(hip_device):
    dev = hip_device
    both, alone, W, rgb = M.two_sphere_fields()
    two, one = _volume_mesh(dev, both, W, rgb), _volume_mesh(dev, alone, W, rgb)
    lab = ops.meshComponents(dev, two)
    _assert_labels(lab, M.components(two["faces"], two["vertices"].shape[0]), "two spheres")
    assert lab["count"] == 2 and lab["invalidFaces"] == 0
    for c in range(2):
        topo = t64.mesh_topology(two["faces"][lab["faceComponent"] == c])
        assert topo["closed"] and topo["consistent"] and topo["V"] - topo["E"] + topo["F"] == 2, (c, topo)
        assert topo["V"] == lab["vertices"][c] and topo["F"] == lab["triangles"][c]
    kept = ops.removeSmallComponents(dev, two, keepLargest=1)
    assert one["faces"].shape[0] == int(lab["triangles"].max()) and one["colours"] is not None
    _assert_mesh(kept, one, "keepLargest = 1 vs sphere A alone", ("vertices", "faces", "colours", "keys"))
    small = ops.removeSmallComponents(dev, two, minTriangles=int(lab["triangles"].max()) + 1)
    assert small["faces"].shape == (0, 3) and small["vertices"].shape == (0, 3) and small["keys"].shape == (0,)


# ---------------------------------------------------------------- 4. the Trainer surface
def test_trainer_extract_mesh_and_evaluate_geometry_take_the_selection(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    try:
        for _ in range(4):
            t.step()
        t.drain()
        iteration, rng_state = t.iteration, t._rng.getstate()
        t.fuseDepth(vol)
        parent = ops.weldTriangles(vol.extractTriangles(1.0))   # what extractMesh returned before it took a selection
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == {"vertices", "faces", "colours", "keys"}
        _assert_mesh(raw, parent, "extractMesh with the defaults", ("vertices", "faces", "colours", "keys"))
        _assert_mesh(t.extractMesh(lo, hi, voxel, keepLargest=None, minTriangles=0, minFraction=0.0), parent, "the defaults spelled out",
                     ("vertices", "faces", "colours", "keys"))
        lab = ops.meshComponents(dev, raw)
        assert lab["count"] >= 2, "the scene's level set has floaters"
        for kw in (dict(keepLargest=1), dict(minTriangles=20), dict(minFraction=0.05)):
            got, want = t.extractMesh(lo, hi, voxel, **kw), ops.removeSmallComponents(dev, raw, **kw)
            _assert_mesh(got, want, f"extractMesh {kw}", MESH_KEYS + ("colours", "keys"))
            _assert_mesh(want, M.remove_small(raw, **kw), f"removeSmallComponents {kw} vs the restatement", MESH_KEYS + ("colours", "keys"))
        assert t.iteration == iteration and t._rng.getstate() == rng_state
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        r = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1)
        mesh = t.extractMesh(lo, hi, voxel, keepLargest=1)
        samples = ops.sampleMesh(dev, mesh, 1.0 / (voxel / 2) ** 2, 0)["points"]
        hand = ops.geometryMetrics(dev, samples, reference, 8.0, 0.5)
        assert r["faces"] == mesh["faces"].shape[0] == int(lab["triangles"].max()) and r["vertices"] == mesh["vertices"].shape[0] and r["samples"] == samples.shape[0]
        _same_metrics({k: r[k] for k in hand}, hand, "evaluateGeometry(keepLargest=1) vs the three calls by hand")
        everything = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5)
        assert everything["faces"] == raw["faces"].shape[0] > r["faces"]
    finally:
        vol.destroy()
        t.destroy()
