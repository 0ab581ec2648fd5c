"""GPU: mesh adjacency, Taubin smoothing and vertex normals on the device (csrc/meshadjacency.hip).  Every output byte equals the
restatement (tests/meshsmooth_ref.py) on its crafted meshes -- empty inputs, degenerate topology, bad indices, non-finite positions, long rows, long runs of
unused vertices, the sort's tile edges, a face count of several scan blocks -- then the iteration counts and both parities of the ping-pong, capacity,
state and argument errors, recording, repeats and reuse, the two-sphere TSDF volume, and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshclean_ref as M
import meshsmooth_ref as R
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


def _upload(dev, m):
    return dict(vertices=dev.bufferFrom(m["vertices"]), faces=dev.bufferFrom(m["faces"]), V=m["vertices"].shape[0], F=m["faces"].shape[0])


def _run(dev, adj, m, smoothing=None, in_place=False):
    """Everything one ``MeshAdjacency`` gives for ``m``: ``dict(rowStart, neighbours, boundary, stats, smoothed, normals)`` -- the normals of the
    unsmoothed positions, as the restatement's ``expected``."""
    src = _upload(dev, m)
    V, F = src["V"], src["F"]
    sm = dict(m["smoothing"] if smoothing is None else smoothing)
    E = adj.count(src["faces"], F, V)
    outs = dict(rowStart=dev.createBuffer(4 * (V + 1)), neighbours=dev.createBuffer(4 * E), boundary=dev.createBuffer(4 * V), normals=dev.createBuffer(12 * V),
                smoothed=dev.createBuffer(12 * V))
    adj.emit(outs["rowStart"], outs["neighbours"], outs["boundary"])
    adj.normals(src["vertices"], src["faces"], V, F, outs["normals"])
    target = src["vertices"] if in_place else outs["smoothed"]
    adj.smooth(src["vertices"], target, V, sm["iterations"], sm["lam"], sm["mu"], sm["pin_boundary"])
    got = dict(rowStart=outs["rowStart"].read(np.uint32, count=V + 1), neighbours=outs["neighbours"].read(np.uint32, count=E),
               boundary=outs["boundary"].read(np.uint32, count=V), normals=outs["normals"].read(np.float32, count=3 * V).reshape(V, 3),
               smoothed=target.read(np.float32, count=3 * V).reshape(V, 3), stats=adj.stats())
    dev.synchronize()
    for b in list(outs.values()) + [src["vertices"], src["faces"]]:
        b.destroy()
    return got


def _assert_result(got, want, what, keys=R.OUTPUTS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")
    assert got["stats"] == want["stats"], f"{what}: {got['stats']}"


# ---------------------------------------------------------------- 1. the crafted meshes
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_device_adjacency_smoothing_and_normals_equal_the_restatement(hip_device, name):
    dev = hip_device
    m, want = R.case(name), R.expected(name)
    adj = ops.MeshAdjacency(dev)
    try:
        got = _run(dev, adj, m)
    finally:
        adj.destroy()
    _assert_result(got, want, name)
    for k, n in R.EXPECT.get(name, {}).items():
        assert got["stats"][k] == n, f"{name}: {k}"
    assert R.digest(got) == R.digest(want)
    # the one-call forms
    one = ops.meshAdjacency(dev, m)
    _assert_result(dict(one, smoothed=want["smoothed"], normals=want["normals"]), want, f"meshAdjacency: {name}")
    sm = m["smoothing"]
    smoothed = ops.smoothMesh(dev, dict(m, colours=None), sm["iterations"], sm["lam"], sm["mu"], sm["pin_boundary"])
    assert_bits_equal(smoothed["vertices"], want["smoothed"], f"smoothMesh: {name}")
    assert smoothed["stats"] == want["stats"] and smoothed["faces"] is m["faces"] and smoothed["colours"] is None
    assert_bits_equal(ops.vertexNormals(dev, m), want["normals"], f"vertexNormals: {name}")


@pytest.mark.parametrize("name", ["noisy-icosphere", "grid-pinned", "non-finite", "fan-65", "two-triangles"])
def test_iteration_counts_weights_and_both_parities_of_the_ping_pong(hip_device, name):
    dev = hip_device
    m = R.case(name)
    adjacency = R.adjacency(m["faces"], m["vertices"].shape[0])
    adj = ops.MeshAdjacency(dev)
    try:
        for iterations in (0, 1, 2, 3):
            for lam, mu in ((0.5, -0.53), (0.5, 0.0), (0.0, -0.53), (0.0, 0.0), (0.33, 0.34)):
                for pin in (True, False):
                    sm = dict(iterations=iterations, lam=lam, mu=mu, pin_boundary=pin)
                    want = R.smooth(m["vertices"], m["faces"], adj=adjacency, **sm)
                    for in_place in (False, True):
                        got = _run(dev, adj, m, sm, in_place)
                        assert_bits_equal(got["smoothed"], want, f"{name}: {sm}, in place: {in_place}")
    finally:
        adj.destroy()


def test_normals_of_smoothed_positions_and_the_sphere(hip_device):
    dev = hip_device
    m, want = R.case("noisy-icosphere"), R.expected("noisy-icosphere")
    got = ops.vertexNormals(dev, dict(vertices=want["smoothed"], faces=m["faces"]))
    assert_bits_equal(got, R.normals(want["smoothed"], m["faces"]), "normals of the smoothed sphere")
    assert np.all(np.sum(got.astype(np.float64) * want["smoothed"], axis=1) > 0)
    v, f = R.noisy_icosphere()
    radius = lambda p: np.linalg.norm(np.asarray(p, np.float64), axis=1)
    taubin, laplace = radius(ops.smoothMesh(dev, dict(vertices=v, faces=f))["vertices"]), radius(ops.smoothMesh(dev, dict(vertices=v, faces=f), mu=0.0)["vertices"])
    before = radius(np.asarray(v, np.float32))
    assert taubin.std() < before.std() and abs(taubin.mean() - before.mean()) < abs(laplace.mean() - before.mean())


# ---------------------------------------------------------------- 2. errors, recording, repeats
def test_capacity_state_arguments_and_recording(hip_device):
    dev = hip_device
    m, want = R.case("tile-above"), R.expected("tile-above")
    src = _upload(dev, m)
    V, F, E = src["V"], src["F"], want["neighbours"].shape[0]
    outs = dict(rowStart=dev.createBuffer(4 * (V + 1)), neighbours=dev.createBuffer(4 * E), boundary=dev.createBuffer(4 * V))
    smoothed, normals = dev.createBuffer(12 * V), dev.createBuffer(12 * V)
    adj = ops.MeshAdjacency(dev)
    sm = m["smoothing"]
    smooth = lambda: adj.smooth(src["vertices"], smoothed, V, sm["iterations"], sm["lam"], sm["mu"], sm["pin_boundary"])
    try:
        for call in (adj.stats, lambda: adj.emit(outs["rowStart"], outs["neighbours"], outs["boundary"], E), smooth,
                     lambda: adj.normals(src["vertices"], src["faces"], V, F, normals)):
            with pytest.raises(_lib.StateError):   # no count precedes it
                call()
        assert adj.count(src["faces"], F, V) == E
        for b in list(outs.values()) + [smoothed, normals]:
            b.write(np.full(b.size // 4, SENTINEL, np.uint32))
        for cap in (E - 1, 0):
            with pytest.raises(_lib.CapacityError):
                adj.emit(outs["rowStart"], outs["neighbours"], outs["boundary"], cap)
        with pytest.raises(_lib.StateError):   # another V
            adj.smooth(src["vertices"], smoothed, V - 1, 1)
        with pytest.raises(_lib.StateError):
            adj.normals(src["vertices"], src["faces"], V - 1, F, normals)
        with pytest.raises(_lib.StateError):
            adj.normals(src["vertices"], src["faces"], V, F - 1, normals)
        other = dev.bufferFrom(m["faces"])
        with pytest.raises(_lib.StateError):   # faces that were not counted
            adj.normals(src["vertices"], other, V, F, normals)
        for lam, mu, it in ((float("nan"), 0.5, 1), (0.5, float("inf"), 1), (float("-inf"), 0.0, 0), (0.5, -0.53, 1025), (0.5, -0.53, 2 ** 31)):
            with pytest.raises(_lib.WdgsError) as e:
                adj.smooth(src["vertices"], smoothed, V, it, lam, mu)
            assert e.value.code == _lib.WDGS_E_INVALID, (lam, mu, it)
        dev.synchronize()
        for k, b in dict(outs, smoothed=smoothed, normals=normals).items():
            assert np.all(b.read(np.uint32) == SENTINEL), f"a refused call wrote {k}"
        adj.emit(None, None, None)   # every output is optional
        adj.emit(outs["rowStart"])
        assert_bits_equal(outs["rowStart"].read(np.uint32), want["rowStart"], "emit of the row starts alone")
        assert np.all(outs["neighbours"].read(np.uint32) == SENTINEL) and np.all(outs["boundary"].read(np.uint32) == SENTINEL)
        adj.emit(outs["rowStart"], outs["neighbours"], outs["boundary"])
        smooth()
        adj.normals(src["vertices"], src["faces"], V, F, normals)
        read = lambda: dict(rowStart=outs["rowStart"].read(np.uint32), neighbours=outs["neighbours"].read(np.uint32), boundary=outs["boundary"].read(np.uint32),
                            smoothed=smoothed.read(np.float32).reshape(V, 3), normals=normals.read(np.float32).reshape(V, 3), stats=adj.stats())
        eager = read()
        _assert_result(eager, want, "after the refusals")
        # emit, smooth and normals wait for nothing and record
        for b in list(outs.values()) + [smoothed, normals]:
            b.clear()
        with dev.createCommandEncoder("adjacency", record=True) as enc:
            adj.emit(outs["rowStart"], outs["neighbours"], outs["boundary"])
            smooth()
            adj.normals(src["vertices"], src["faces"], V, F, normals)
            cmd = enc.finish()
        assert np.all(smoothed.read(np.uint32) == 0) and np.all(outs["neighbours"].read(np.uint32) == 0), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        _assert_result(read(), eager, "recorded and replayed")
        cmd.destroy()
        with pytest.raises(_lib.StateError):   # the count waits for its totals
            with dev.createCommandEncoder("doomed", record=True):
                adj.count(src["faces"], F, V)
        dev.synchronize()
        with pytest.raises(_lib.StateError):   # a refused count leaves nothing to emit
            adj.emit(outs["rowStart"])
        for nv, nf in ((2 ** 31, 1), (1, 2 ** 32 // 6 + 1)):
            with pytest.raises(_lib.WdgsError) as e:
                adj.count(src["faces"], nf, nv)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.WdgsError):
            adj.count(None, 3, 3)
    finally:
        adj.destroy()
        adj.destroy()   # idempotent


def test_two_runs_agree_and_one_object_takes_meshes_of_any_size(hip_device):
    dev = hip_device
    m = R.case("many-faces")
    sm = m["smoothing"]
    a, b = (ops.smoothMesh(dev, m, sm["iterations"], pinBoundary=False) for _ in range(2))
    assert_bits_equal(b["vertices"], a["vertices"], "a second run")
    assert_bits_equal(ops.vertexNormals(dev, m), ops.vertexNormals(dev, m), "a second run of the normals")
    adj = ops.MeshAdjacency(dev)
    try:
        for name in ("two-triangles", "random", "many-faces", "no-faces", "fan-5000", "nothing", "tail-used", "no-vertices", "tile-below", "tetrahedron"):
            _assert_result(_run(dev, adj, R.case(name)), R.expected(name), f"reused object: {name}")
    finally:
        adj.destroy()


def test_one_count_is_one_sort_launch_for_launch(hip_device):
    """The launch sequence of count + emit + two iterations + normals, pinned: ONE stable u64 sort (csrc/keysort.hip) -- its plan, eight histogram and
    scatter launches, head flags -- each adjacency kernel once, four smoothing steps, and the library scan ten times: eight digit tables, the head flags,
    the degrees."""
    dev = hip_device
    m = R.case("random")
    src = _upload(dev, m)
    V, F = src["V"], src["F"]
    adj = ops.MeshAdjacency(dev)
    try:
        outs = [dev.createBuffer(4 * (V + 1)), dev.createBuffer(24 * F), dev.createBuffer(4 * V), dev.createBuffer(12 * V), dev.createBuffer(12 * V)]
        dev.synchronize()
        dev.setProfiling(True)
        dev.kernelTimes(reset=True)
        adj.count(src["faces"], F, V)
        adj.emit(outs[0], outs[1], outs[2])
        adj.smooth(src["vertices"], outs[3], V, 2)
        adj.normals(src["vertices"], src["faces"], V, F, outs[4])
        dev.synchronize()
        dev.setProfiling(False)
        times = dev.kernelTimes(reset=True)
    finally:
        dev.setProfiling(False)
        adj.destroy()
    launches = {k: v[0] for k, v in times.items()}
    print("launches:", sorted(launches.items()))
    assert {k: n for k, n in launches.items() if k.startswith("weld_")} == dict(weld_key_bits=1, weld_plan=1, weld_histogram=8, weld_scatter=8, weld_heads=1), launches
    assert {k: n for k, n in launches.items() if k.startswith("adjacency_")} == dict(adjacency_half_edge_keys=1, adjacency_fold=1, adjacency_edges=1, adjacency_rows=1,
                                                                                       adjacency_emit=1, adjacency_smooth_step=4, adjacency_vertex_normals=1), launches
    assert {k: n for k, n in launches.items() if k.startswith("scan_")} == dict(scan_reduce=10, scan_block_sums=10, scan_downsweep=10), launches


# ---------------------------------------------------------------- 3. two spheres in a TSDF volume
def _assert_mesh(got, want, what):
    assert list(got) == list(want), f"{what}: {list(got)}"
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}"
            assert_bits_equal(got[k], w, f"{what}: {k}")
        else:
            assert got[k] == w, f"{what}: {k} = {got[k]}"


def test_two_sphere_volume_smooths_to_the_restatement(hip_device):
    dev = hip_device
    both, _, wt, rgb = M.two_sphere_fields()
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    cell = 2.0 * M.TS_VOXEL
    welded = smoothed = {}
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        host = vol.extractMesh()
        V, F = host["vertices"].shape[0], host["faces"].shape[0]
        adjacency = R.adjacency(host["faces"], V)
        st = adjacency["stats"]
        print(f"two-sphere mesh: V={V} F={F} stats={st} Euler characteristic={V - st['edges'] + F - st['invalidFaces']}")
        want_v = R.smooth(host["vertices"], host["faces"], 3, adj=adjacency)
        mine = ops.smoothMesh(dev, host, 3)
        assert list(mine) == ["vertices", "faces", "colours", "keys", "stats"] and mine["stats"] == st
        assert_bits_equal(mine["vertices"], want_v, "smoothMesh of extractMesh()")
        for k in ("faces", "colours", "keys"):
            assert mine[k] is host[k]
        normals = ops.vertexNormals(dev, mine)
        assert_bits_equal(normals, R.normals(want_v, host["faces"], adj=adjacency), "vertexNormals of the smoothed mesh")
        want = dict(mine, normals=normals)
        for weld in ("device", "host"):
            _assert_mesh(vol.extractMesh(weld=weld, smooth=3, normals=True), want, f"extractMesh(weld={weld!r}, smooth=3, normals=True)")
        _assert_mesh(vol.extractMesh(weld="device", normals=True), dict(host, normals=ops.vertexNormals(dev, host)), "extractMesh(normals=True)")
        simplified = ops.simplifyMesh(dev, mine, cell, origin=M.TS_ORIGIN)
        for weld in ("device", "host"):
            _assert_mesh(vol.extractMesh(weld=weld, smooth=3, simplify=cell), simplified, f"extractMesh(weld={weld!r}, smooth=3, simplify=)")
            _assert_mesh(vol.extractMesh(weld=weld, smooth=3, simplify=cell, normals=True), dict(simplified, normals=ops.vertexNormals(dev, simplified)),
                         f"extractMesh(weld={weld!r}, smooth=3, simplify=, normals=True)")
        for weld in ("device", "host"):
            again = vol.extractMesh(weld=weld, smooth=None, normals=False)
            assert set(again) == {"vertices", "faces", "colours", "keys"}
            for k in again:
                assert_bits_equal(again[k], host[k], f"smooth=None, normals=False: {k}")
        # a mesh of buffers in, and out
        tri = vol.extractTriangleBuffers()
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        ops.destroyBuffers(tri)
        smoothed = ops.smoothMesh(dev, welded, 3, asBuffers=True)
        assert smoothed["vertices"] is not welded["vertices"] and smoothed["faces"] is welded["faces"] and smoothed["vertices"].size == 12 * V
        assert_bits_equal(smoothed["vertices"].read(np.float32).reshape(V, 3), want_v, "asBuffers: vertices")
        assert_bits_equal(welded["vertices"].read(np.float32).reshape(V, 3), host["vertices"], "the input is left as it is")
        _assert_mesh(ops.simplifyMesh(dev, smoothed, cell, origin=M.TS_ORIGIN), simplified, "asBuffers into simplifyMesh")
        assert_bits_equal(ops.vertexNormals(dev, smoothed), normals, "asBuffers into vertexNormals")
        twice = ops.smoothMesh(dev, ops.simplifyMesh(dev, welded, cell, origin=M.TS_ORIGIN), 2)   # simplifyMesh's dict into smoothMesh
        assert twice["stats"]["directedEdges"] > 0 and "faceMap" in twice
    finally:
        if smoothed:
            smoothed["vertices"].destroy()
        ops.destroyBuffers(welded)
        vol.destroy()


# ---------------------------------------------------------------- 4. the Trainer surface
def test_trainer_extract_mesh_smooths_before_it_simplifies(hip_device):
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
        raw = t.extractMesh(lo, hi, voxel, smooth=None, normals=False)
        assert set(raw) == {"vertices", "faces", "colours", "keys"} and raw["faces"].shape[0] > 0
        for k in raw:
            assert_bits_equal(raw[k], parent[k], f"the defaults still equal the parent's output: {k}")
        smoothed = ops.smoothMesh(dev, raw, 3)
        assert np.any(smoothed["vertices"] != raw["vertices"])
        want = dict(smoothed, normals=ops.vertexNormals(dev, smoothed))
        for weld in ("host", "device"):
            _assert_mesh(t.extractMesh(lo, hi, voxel, weld=weld, smooth=3, normals=True), want, f"extractMesh(weld={weld!r}, smooth=3, normals=True)")
        want_simplified = ops.simplifyMesh(dev, smoothed, cell, origin=vol.origin)
        for weld in ("host", "device"):
            _assert_mesh(t.extractMesh(lo, hi, voxel, weld=weld, smooth=3, simplify=cell), want_simplified, f"extractMesh(weld={weld!r}, smooth=3, simplify=)")
        largest = t.extractMesh(lo, hi, voxel, keepLargest=1)
        assert largest["faces"].shape[0] < raw["faces"].shape[0], "the scene's level set has floaters"
        smoothed1 = ops.smoothMesh(dev, largest, 3)
        want1 = dict(smoothed1, normals=ops.vertexNormals(dev, smoothed1))
        simplified1 = ops.simplifyMesh(dev, smoothed1, cell, origin=vol.origin)
        want1s = dict(simplified1, normals=ops.vertexNormals(dev, simplified1))
        for weld in ("host", "device"):
            _assert_mesh(t.extractMesh(lo, hi, voxel, keepLargest=1, weld=weld, smooth=3, normals=True), want1, f"extractMesh(keepLargest=1, weld={weld!r}, smooth=3)")
            _assert_mesh(t.extractMesh(lo, hi, voxel, keepLargest=1, weld=weld, smooth=3, simplify=cell, normals=True), want1s,
                         f"extractMesh(keepLargest=1, weld={weld!r}, smooth=3, simplify=, normals=True)")
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        for weld in ("host", "device"):
            out = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1, weld=weld, smooth=3)
            assert (out["vertices"], out["faces"]) == (want1["vertices"].shape[0], want1["faces"].shape[0])
            for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore"):
                assert np.isfinite(out[k]), f"evaluateGeometry(smooth=): {k} = {out[k]}"
        assert t.iteration == iteration and t._rng.getstate() == rng_state
    finally:
        vol.destroy()
        t.destroy()
