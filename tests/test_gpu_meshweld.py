"""GPU: welding a triangle soup on the device (csrc/meshweld.hip over the sort of csrc/keysort.hip).  Every output byte equals ``ops.weldTriangles`` on the same soup: the
crafted soups of tests/meshweld_ref.py (sizes and edge values, pass skipping, load and duplication, the lowest-slot rule, a digit table of several scan blocks),
capacity and state errors, recording, repeats and reuse, the two-sphere TSDF volume, and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshclean_ref as M
import meshweld_ref as W
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views
from test_gpu_geometry import _same_metrics

pytestmark = pytest.mark.gpu

KEYS = ("vertices", "faces", "colours", "keys")
SENTINEL = 0xA5A5A5A5


def _assert_mesh(got, want, what, keys=KEYS):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, f"{what}: {k}"
            continue
        assert got[k].dtype == want[k].dtype, f"{what}: {k} is {got[k].dtype}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


def _upload(dev, tri):
    return dict(keys=dev.bufferFrom(tri["keys"]), positions=dev.bufferFrom(tri["positions"]), colours=dev.bufferFrom(tri["colours"]),
                numTriangles=tri["keys"].shape[0])


def _read(outs, V, F):
    return dict(vertices=outs["vertices"].read(np.float32, count=3 * V).reshape(V, 3), faces=outs["faces"].read(np.uint32, count=3 * F).reshape(F, 3),
                colours=np.ascontiguousarray(outs["colours"].read(np.uint8, count=4 * V).reshape(V, 4)[:, :3]), keys=outs["keys"].read(np.uint64, count=V))


def _outputs(dev, V, F):
    return dict(vertices=dev.createBuffer(12 * V), faces=dev.createBuffer(12 * F), colours=dev.createBuffer(4 * V), keys=dev.createBuffer(8 * V))


def _emit(welder, src, outs, **kw):
    welder.emit(src["keys"], 3 * src["numTriangles"], src["positions"], src["colours"], outs["faces"], outs["vertices"], outs["colours"], outs["keys"], **kw)


def _weld_with(dev, welder, tri):
    """The welded mesh of ``tri`` through ``welder``, and the count's statistics."""
    src = _upload(dev, tri)
    F = src["numTriangles"]
    V = welder.count(src["keys"], 3 * F)
    outs = _outputs(dev, V, F)
    _emit(welder, src, outs)
    mesh = _read(outs, V, F)
    dev.synchronize()
    return mesh, welder.stats()


# ---------------------------------------------------------------- 1. the crafted soups
@pytest.mark.parametrize("name", sorted(W.CASES))
def test_device_weld_equals_weld_triangles(hip_device, name):
    dev = hip_device
    tri = W.case(name)
    want = ops.weldTriangles(tri)
    welder = ops.MeshWelder(dev)
    try:
        got, stats = _weld_with(dev, welder, tri)
    finally:
        welder.destroy()
    _assert_mesh(got, want, name)
    V, S = want["keys"].shape[0], tri["keys"].size
    assert (stats["vertices"], stats["slots"]) == (V, S) and stats["passesRun"] + stats["passesSkipped"] == 8, stats
    if name in W.PASSES_RUN:
        assert stats["passesRun"] == W.PASSES_RUN[name], f"{name}: {stats}"
    _assert_mesh(ops.weldTrianglesDevice(dev, tri), want, f"weldTrianglesDevice: {name}")


def test_expected_vertex_counts_of_the_edge_cases(hip_device):
    for name, V in (("empty", 0), ("one-distinct", 3), ("one-equal", 1), ("all-equal", 1), ("lowest-slot", 4)):
        got = ops.weldTrianglesDevice(hip_device, W.case(name))
        assert got["keys"].shape == (V,) and got["vertices"].shape == (V, 3) and got["colours"].shape == (V, 3), name
    tri = W.case("extremes")
    got = ops.weldTrianglesDevice(hip_device, tri)
    assert got["keys"][0] == 0 and got["keys"][-1] == np.uint64(W.U64_MAX)
    bare = dict(keys=tri["keys"], positions=tri["positions"], colours=None)
    _assert_mesh(ops.weldTrianglesDevice(hip_device, bare), ops.weldTriangles(bare), "a soup without colours")


def test_lowest_slot_rule(hip_device):
    tri = W.case("lowest-slot")
    got = ops.weldTrianglesDevice(hip_device, tri)
    keys = tri["keys"].reshape(-1)
    first = np.array([np.flatnonzero(keys == k)[0] for k in got["keys"]])
    assert_bits_equal(got["vertices"], np.repeat(first.astype(np.float32), 3).reshape(-1, 3), "every vertex is its lowest slot's position")
    assert_bits_equal(got["colours"], tri["colours"].reshape(-1, 4)[first, :3], "every vertex is its lowest slot's colour")


# ---------------------------------------------------------------- 2. errors, recording, repeats
def test_capacity_state_and_argument_errors(hip_device):
    dev = hip_device
    tri = W.case("random-u64")
    want = ops.weldTriangles(tri)
    V, F = want["keys"].shape[0], tri["keys"].shape[0]
    src = _upload(dev, tri)
    outs = _outputs(dev, V, F)
    welder = ops.MeshWelder(dev)
    try:
        with pytest.raises(_lib.StateError):
            welder.stats()
        with pytest.raises(_lib.StateError):   # no count precedes it
            _emit(welder, src, outs)
        assert welder.count(src["keys"], 3 * F) == V
        for b in outs.values():
            b.write(np.full(b.size // 4, SENTINEL, np.uint32))
        for cap in (V - 1, 0):
            with pytest.raises(_lib.CapacityError):
                _emit(welder, src, outs, capacity=cap)
        with pytest.raises(_lib.StateError):   # a count of other arguments
            welder.emit(src["keys"], 3 * F - 3, src["positions"], src["colours"], outs["faces"], outs["vertices"], outs["colours"], outs["keys"])
        other = dev.bufferFrom(tri["keys"])
        with pytest.raises(_lib.StateError):
            welder.emit(other, 3 * F, src["positions"], src["colours"], outs["faces"], outs["vertices"], outs["colours"], outs["keys"])
        dev.synchronize()
        for k, b in outs.items():
            assert np.all(b.read(np.uint32) == SENTINEL), f"a refused emit wrote {k}"
        _emit(welder, src, outs)
        eager = _read(outs, V, F)
        _assert_mesh(eager, want, "emit after the refusals")
        # faces alone
        outs["faces"].clear()
        welder.emit(src["keys"], 3 * F, None, None, outs["faces"])
        assert_bits_equal(outs["faces"].read(np.uint32).reshape(F, 3), want["faces"], "emit without vertices: faces")
        # the emit waits for nothing and records
        for b in outs.values():
            b.clear()
        with dev.createCommandEncoder("weld emit", record=True) as enc:
            _emit(welder, src, outs)
            cmd = enc.finish()
        assert np.all(outs["faces"].read(np.uint32) == 0), "recording runs nothing"
        dev.queue.submit([cmd])
        dev.synchronize()
        _assert_mesh(_read(outs, V, F), eager, "a recorded emit, replayed")
        cmd.destroy()
        with pytest.raises(_lib.StateError):   # the count waits for V
            with dev.createCommandEncoder("doomed", record=True):
                welder.count(src["keys"], 3 * F)
        dev.synchronize()
        for bad in (3 * F - 1, 2 ** 32, 2 ** 32 + 2, 3 * 2 ** 31):
            with pytest.raises(_lib.WdgsError) as e:
                welder.count(src["keys"], bad)
            assert e.value.code == _lib.WDGS_E_INVALID, bad
        with pytest.raises(_lib.WdgsError):
            welder.count(None, 3)
        with pytest.raises(_lib.StateError):   # a refused count leaves nothing to emit
            _emit(welder, src, outs)
    finally:
        welder.destroy()
        welder.destroy()   # idempotent
    with pytest.raises(ValueError):
        ops.weldTrianglesDevice(dev, dict(keys=np.zeros(4, np.uint64), positions=np.zeros((4, 3), np.float32), colours=None))


def test_two_runs_agree_and_one_welder_takes_soups_of_any_size(hip_device):
    dev = hip_device
    a, b = ops.weldTrianglesDevice(dev, W.case("scan-blocks")), ops.weldTrianglesDevice(dev, W.case("scan-blocks"))
    _assert_mesh(b, a, "a second run")
    welder = ops.MeshWelder(dev)
    try:
        for name in ("one-distinct", "random-u64", "scan-blocks", "extremes", "empty", "heavy-bin", "all-equal"):
            got, _ = _weld_with(dev, welder, W.case(name))
            _assert_mesh(got, ops.weldTriangles(W.case(name)), f"reused welder: {name}")
    finally:
        welder.destroy()


# The launches of one stable u64 sort; histogram and scatter launch for every one of the eight passes, and a pass the plan skips returns at once
SORT_LAUNCHES = dict(weld_key_bits=1, weld_plan=1, weld_histogram=8, weld_scatter=8, weld_heads=1, weld_emit=1)


def test_one_weld_is_one_sort_launch_for_launch(hip_device):
    """The launch sequence of one count + emit, pinned: the six sort labels once per sort (the two per-pass ones eight times), and the library scan's
    three kernels nine times each -- eight digit tables and the head flags.  The scan_* literals are what the library gave on this soup before the
    sort moved into csrc/keysort.hip; the sort's follow from its code."""
    dev = hip_device
    tri = W.case("random-u64")
    assert tri["keys"].size == 20481
    src = _upload(dev, tri)
    F = src["numTriangles"]
    welder = ops.MeshWelder(dev)
    try:
        outs = _outputs(dev, 3 * F, F)
        dev.synchronize()
        dev.setProfiling(True)
        dev.kernelTimes(reset=True)
        welder.count(src["keys"], 3 * F)
        _emit(welder, src, outs)
        dev.synchronize()
        dev.setProfiling(False)
        times = dev.kernelTimes(reset=True)
        stats = welder.stats()
    finally:
        dev.setProfiling(False)
        welder.destroy()
    launches = {k: v[0] for k, v in times.items()}
    print("launches:", sorted(launches.items()))
    assert {k: n for k, n in launches.items() if k.startswith("weld_")} == SORT_LAUNCHES, launches
    assert {k: n for k, n in launches.items() if k.startswith("scan_")} == dict(scan_reduce=9, scan_block_sums=9, scan_downsweep=9), launches
    assert stats["passesRun"] == 8, stats


# ---------------------------------------------------------------- 3. two spheres in a TSDF volume
def test_two_sphere_volume_welds_to_the_host_mesh(hip_device):
    dev = hip_device
    both, _, wt, rgb = M.two_sphere_fields()
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    welded = None
    try:
        vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
        vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
        vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
        host = vol.extractMesh()
        _assert_mesh(host, ops.weldTriangles(vol.extractTriangles()), "the default is the host weld")
        _assert_mesh(vol.extractMesh(weld="device"), host, "extractMesh(weld='device')")
        with pytest.raises(ValueError):
            vol.extractMesh(weld="somewhere")
        tri = vol.extractTriangleBuffers()
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        ops.destroyBuffers(tri)
        assert (welded["numVertices"], welded["numFaces"]) == (host["vertices"].shape[0], host["faces"].shape[0])
        want = ops.removeSmallComponents(dev, host, keepLargest=1)
        got = ops.removeSmallComponents(dev, dict(vertices=welded["vertices"], faces=welded["faces"]), keepLargest=1)
        _assert_mesh(got, want, "asBuffers into removeSmallComponents", ("vertices", "faces", "vertexMap", "faceMap", "components"))
        lab = ops.meshComponents(dev, dict(vertices=welded["vertices"], faces=welded["faces"]))
        assert lab["count"] == 2 and lab["invalidFaces"] == 0
        a = ops.sampleMesh(dev, dict(vertices=welded["vertices"], faces=welded["faces"]), 50.0, 3)
        b = ops.sampleMesh(dev, host, 50.0, 3)
        assert_bits_equal(a["points"], b["points"], "asBuffers into sampleMesh")
    finally:
        if welded is not None:
            ops.destroyBuffers(welded)
        vol.destroy()


# ---------------------------------------------------------------- 4. the Trainer surface
def test_trainer_extract_mesh_welds_on_the_device(hip_device):
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
        parent = ops.weldTriangles(vol.extractTriangles(1.0))
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == {"vertices", "faces", "colours", "keys"} and raw["faces"].shape[0] > 0
        _assert_mesh(raw, parent, "extractMesh with the defaults")
        _assert_mesh(t.extractMesh(lo, hi, voxel, weld="device"), raw, "extractMesh(weld='device')")
        want = t.extractMesh(lo, hi, voxel, keepLargest=1)
        got = t.extractMesh(lo, hi, voxel, keepLargest=1, weld="device")
        assert list(got) == list(want)
        _assert_mesh(got, want, "extractMesh(keepLargest=1, weld='device')", ("vertices", "faces", "vertexMap", "faceMap", "components", "colours", "keys"))
        assert want["faces"].shape[0] < raw["faces"].shape[0], "the scene's level set has floaters"
        with pytest.raises(ValueError):
            t.extractMesh(lo, hi, voxel, weld="somewhere")
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        a = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1)
        b = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, keepLargest=1, weld="device")
        a.pop("ms"), b.pop("ms")
        _same_metrics(b, a, "evaluateGeometry(weld='device')")
        assert t.iteration == iteration and t._rng.getstate() == rng_state
    finally:
        vol.destroy()
        t.destroy()
