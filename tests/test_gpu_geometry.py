"""GPU: mesh accuracy metrics (csrc/geometry.hip).  Surface sampling, the point index's nearest-point queries and the distance sums
against the float32 restatement (tests/geometry_ref.py), byte for byte; state, capacity and argument errors; cell-size independence; recording; the metrics on
the CPU tests' sampled planes; and the Trainer surface."""
import numpy as np
import pytest

from webdgs_amd import _lib, loaders, ops

import geometry_ref as G
import harness
import test_geometry_reference as R
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

MARK = 0x7FC01234


# ---------------------------------------------------------------- helpers
def _assert_samples_equal(dev, v, f, density, seed, what):
    got = ops.sampleMesh(dev, dict(vertices=v, faces=f), density, seed)
    want = G.sample_mesh(v, f, density, seed)
    assert got["points"].shape == (want["total"], 3), f"{what}: {got['points'].shape[0]} samples, the restatement has {want['total']}"
    assert_bits_equal(got["face"], want["face"], f"{what}: face")
    assert_bits_equal(got["points"], want["points"], f"{what}: points")
    return got, want


def _assert_nearest_equal(dev, pts, qs, cutoff, cells, what, want=None):
    """The index built with each cell edge of ``cells`` gives the restatement's bytes."""
    want = G.nearest(pts, qs, cutoff) if want is None else want
    for cell in cells:
        index = ops.PointIndex(dev, pts, cellSize=cell)
        try:
            got = index.nearest(qs, cutoff)
            info = index.info()
            assert_bits_equal(got["index"], want[1], f"{what}, cell edge {cell} (grid {info['dims']}): index")
            assert_bits_equal(got["d2"], want[0], f"{what}, cell edge {cell} (grid {info['dims']}): d2")
        finally:
            index.destroy()
    return want


def _same_metrics(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        a, b = got[k], want[k]
        assert (a == b) or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), f"{what}: {k} = {a!r}, the restatement has {b!r}"


# ---------------------------------------------------------------- 1. sampling
def test_sampling_matches_the_restatement(hip_device):
    dev = hip_device
    v, f = G.square_mesh(12, size=3.0)
    v = (v + np.array([0.3, -1.7, 0.9], np.float32)).astype(np.float32)
    v[:, 2] += (0.37 * v[:, 0] - 0.21 * v[:, 1]).astype(np.float32)                 # tilted: every axis takes part
    empty = ops.sampleMesh(dev, dict(vertices=v, faces=np.zeros((0, 3), np.uint32)), 100.0)
    assert empty["points"].shape == (0, 3) and empty["face"].shape == (0,)
    _assert_samples_equal(dev, v, f[:1], 4000.0, 3, "one triangle")
    got, want = _assert_samples_equal(dev, v, f[:257], 900.0, 8, "257 triangles (two workgroups)")
    assert want["total"] > 5000 and np.unique(want["face"]).size == 257
    again = ops.sampleMesh(dev, dict(vertices=v, faces=f[:257]), 900.0, 8)
    assert_bits_equal(again["points"], got["points"], "two runs")
    other = ops.sampleMesh(dev, dict(vertices=v, faces=f[:257]), 900.0, 9)
    assert other["points"].tobytes() != got["points"].tobytes()
    # a density below one sample per triangle: the dither keeps the expected number
    _, sparse = _assert_samples_equal(dev, v, f, 6.0, 1, "sparse")
    assert 0 < sparse["total"] < f.shape[0] and (sparse["counts"] == 0).any()


def test_one_huge_triangle_among_tiny_ones(hip_device):
    """About 50 000 samples on one triangle between 500 tiny ones: the bisection of the scanned offsets and the per-sample emit."""
    tv, tf = G.square_mesh(16, size=0.5)
    tf = tf[:500]
    big = np.array([[0, 0, 1], [10, 0, 1], [0, 10, 2]], np.float32)
    v = np.concatenate([tv, big]).astype(np.float32)
    f = np.concatenate([tf[:250], np.array([[tv.shape[0], tv.shape[0] + 1, tv.shape[0] + 2]], np.uint32), tf[250:]]).astype(np.uint32)
    got, want = _assert_samples_equal(hip_device, v, f, 1000.0, 4, "huge among tiny")
    assert 49000 < want["counts"][250] < 52000 and want["total"] - int(want["counts"][250]) < 3000
    assert (want["counts"][:250] == 0).any() and (want["counts"][:250] > 0).any() and (want["counts"][251:] > 0).any()


def test_degenerate_faces_and_device_meshes(hip_device):
    dev = hip_device
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 5], [0, 0, 0], [0, 1, 4], [2, 1, 0]], np.uint32)
    got, want = _assert_samples_equal(dev, v, f, 1000.0, 3, "degenerate faces")
    assert set(np.unique(got["face"])) == {0, 5}
    # the same mesh handed over as device buffers, and the samples kept on the device
    vb, fb = dev.bufferFrom(v), dev.bufferFrom(f)
    s = ops.sampleMesh(dev, dict(vertices=vb, faces=fb), 1000.0, 3, asBuffers=True)
    assert s["count"] == want["total"]
    assert_bits_equal(s["points"].read(np.float32, count=3 * s["count"]).reshape(-1, 3), want["points"], "device mesh: points")
    with pytest.raises(ValueError):
        ops.sampleMesh(dev, dict(vertices=v[:, :2], faces=f), 10.0)


def test_sampler_state_capacity_and_argument_errors(hip_device):
    dev = hip_device
    v, f = G.square_mesh(4)
    vb, fb = dev.bufferFrom(v), dev.bufferFrom(f)
    nv, nf = v.shape[0], f.shape[0]
    s = ops.MeshSampler(dev)
    out = dev.createBuffer(12 * 4000)
    marker = np.full(3 * 4000, MARK, np.uint32)
    out.write(marker)
    try:
        with pytest.raises(_lib.StateError):                       # no count yet
            s.emit(vb, nv, fb, nf, 1000.0, 1, out)
        total = s.count(vb, nv, fb, nf, 1000.0, 1)
        assert total == G.sample_mesh(v, f, 1000.0, 1)["total"] and 900 < total < 1100
        with pytest.raises(_lib.StateError):                       # another seed, density, face count than the count saw
            s.emit(vb, nv, fb, nf, 1000.0, 2, out)
        with pytest.raises(_lib.StateError):
            s.emit(vb, nv, fb, nf, 1000.5, 1, out)
        with pytest.raises(_lib.StateError):
            s.emit(vb, nv, fb, nf - 1, 1000.0, 1, out)
        with pytest.raises(_lib.CapacityError):                    # too little room
            s.emit(vb, nv, fb, nf, 1000.0, 1, out, capacity=total - 1)
        with pytest.raises(_lib.CapacityError) as e:               # 2^31 samples or more
            s.count(vb, nv, fb, nf, 3.0e9, 1)
        assert "2^31" in str(e.value)
        with pytest.raises(_lib.StateError):                       # ... after which nothing can be emitted
            s.emit(vb, nv, fb, nf, 3.0e9, 1, out)
        dev.synchronize()
        assert_bits_equal(out.read(np.uint32), marker, "a refused emit writes nothing")
        for density in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(_lib.WdgsError) as e:
                s.count(vb, nv, fb, nf, density, 1)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.StateError):                       # the count waits for its total
            with dev.createCommandEncoder("doomed", record=True):
                s.count(vb, nv, fb, nf, 1000.0, 1)
        dev.synchronize()
        total = s.count(vb, nv, fb, nf, 1000.0, 1)
        s.emit(vb, nv, fb, nf, 1000.0, 1, out, capacity=total)     # face is optional
        got = out.read(np.uint32)
        assert np.all(got[3 * total:] == MARK)
        assert_bits_equal(got[:3 * total].view(np.float32).reshape(-1, 3), G.sample_mesh(v, f, 1000.0, 1)["points"], "emit without face")
    finally:
        s.destroy()
        s.destroy()   # idempotent


# ---------------------------------------------------------------- 2. nearest
CLOUD_CUTOFFS = (0.02, 0.09)     # below the mean nearest-neighbour distance of 3 000 points in the unit cube (0.04), and above it


@pytest.mark.parametrize("cutoff", CLOUD_CUTOFFS)
def test_nearest_random_cloud_and_cell_size_independence(hip_device, cutoff):
    pts, qs = R.random_cloud(3000, 21), R.random_cloud(3000, 22)
    want = _assert_nearest_equal(hip_device, pts, qs, cutoff, (cutoff, 2.7 * cutoff, cutoff / 3, None, 1e-9, 50.0), f"3000 x 3000, cutoff {cutoff}")
    found = want[1] != G.NO_INDEX
    assert 0 < found.sum() < 3000 and (found.mean() < 0.5) == (cutoff < 0.04)


def test_nearest_far_beyond_the_cell_edge(hip_device):
    """A cutoff of ten cell edges and more: the ring search ends early for most queries, and must not lose anything by it."""
    pts, qs = R.random_cloud(3000, 21), R.random_cloud(400, 23, scale=1.3) - np.float32(0.15)
    want = _assert_nearest_equal(hip_device, pts, qs, 0.5, (0.05, 0.013, 0.5), "cutoff 0.5")
    assert (want[1] != G.NO_INDEX).all()


def test_nearest_small_sets(hip_device):
    dev = hip_device
    qs = R.random_cloud(70, 31)
    for m in (0, 1, 65):
        _assert_nearest_equal(dev, R.random_cloud(m, 30), qs, 0.4, (0.4, 0.1, None), f"M = {m}")
    index = ops.PointIndex(dev, R.random_cloud(65, 30), cellSize=0.2)
    try:
        empty = index.nearest(np.zeros((0, 3), np.float32), 0.4)
        assert empty["d2"].shape == (0,) and empty["index"].shape == (0,)
        assert index.info()["indexed"] == 65 and index.info()["cellSize"] == pytest.approx(0.2)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(_lib.WdgsError) as e:
                index.nearest(qs, bad)
            assert e.value.code == _lib.WDGS_E_INVALID
    finally:
        index.destroy()
        index.destroy()
    with pytest.raises(_lib.WdgsError) as e:
        ops.PointIndex(dev, R.random_cloud(65, 30), cellSize=-1.0)
    assert e.value.code == _lib.WDGS_E_INVALID
    with pytest.raises(_lib.WdgsError) as e:                       # more than 2^31 - 1 points
        import ctypes
        _lib.check(dev.lib.wdgs_point_index_create(dev.handle, dev.createBuffer(16).ptr, 2 ** 31, 1.0, ctypes.byref(ctypes.c_void_p())))
    assert e.value.code == _lib.WDGS_E_INVALID


def test_identical_points_lowest_index_wins(hip_device):
    pts = np.zeros((300, 3), np.float32) + np.array([0.25, -0.5, 0.125], np.float32)
    qs = np.array([[0.25, -0.5, 0.625], [0.25, -0.5, 0.125], [9, 9, 9]], np.float32)
    want = _assert_nearest_equal(hip_device, pts, qs, 1.0, (1.0, 0.01, None), "300 identical points")
    assert want[1].tolist() == [0, 0, G.NO_INDEX]


def test_lattice_ties_across_cells(hip_device):
    """An integer lattice, shuffled, queried at cell centres (eight equally near points), edge midpoints (two), face centres (four) and the points
    themselves: exact ties between points of different cells -- with the smaller cell edges, of different rings -- and coordinates that are exact
    multiples of the cell edge."""
    g = np.arange(6, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = pts[np.random.default_rng(5).permutation(pts.shape[0])].copy()
    c = np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), axis=-1).reshape(-1, 3)
    qs = np.concatenate([c + np.float32(0.5), c + np.array([0.5, 0, 0], np.float32), c + np.array([0, 0.5, 0.5], np.float32), c]).astype(np.float32)
    for cutoff in (1.0, 0.5, 0.875):          # 0.5: the edge midpoints' two points sit exactly on the cutoff (d2 == r2) and the centres find nothing
        want = _assert_nearest_equal(hip_device, pts, qs, cutoff, (1.0, 0.5, 0.3, 0.37, 2.0, None), f"lattice, cutoff {cutoff}")
        if cutoff >= 0.875:
            assert np.all(want[0][:125] == np.float32(0.75))
            # the winner is the lowest index among the cell's eight corners
            corners = np.array([np.flatnonzero(np.all(np.abs(pts - q) == 0.5, axis=1)).min() for q in qs[:125]])
            assert np.array_equal(want[1][:125].astype(np.int64), corners)
        else:
            assert np.all(want[1][:125] == G.NO_INDEX)
        assert np.all(want[0][125:250] == np.float32(0.25))


def test_queries_outside_the_bounding_box(hip_device):
    """The points fill [0, 1)^3; each group of queries has some coordinates moved outside it, by less and by more than the cutoff of 0.1."""
    pts = R.random_cloud(500, 41)
    inside = R.random_cloud(60, 42)
    moves = [{0: -0.05}, {1: 1.04}, {2: -0.3}, {0: 1.5}, {0: -0.02, 1: -0.03, 2: 1.03}, {0: 100.0, 1: -100.0, 2: 1e6}, {2: 3.0e38}]
    groups = []
    for m in moves:
        q = inside.copy()
        for axis, value in m.items():
            q[:, axis] = value
        groups.append(q)
    qs = np.concatenate(groups).astype(np.float32)
    want = _assert_nearest_equal(hip_device, pts, qs, 0.1, (0.1, 0.03, 0.27, None), "queries outside the box")
    found = (want[1] != G.NO_INDEX).reshape(len(moves), -1)
    assert found[0].any() and found[1].any() and not found[2].any() and not found[3].any() and not found[5].any() and not found[6].any()


def test_one_crowded_cell_and_non_finite_values(hip_device):
    rng = np.random.default_rng(50)
    crowd = (rng.random((5000, 3)) * 0.01 + 0.5).astype(np.float32)
    pts = np.concatenate([R.random_cloud(60, 51), crowd]).astype(np.float32)
    pts[7] = (np.nan, 0.5, 0.5)
    pts[9] = (0.5, np.inf, 0.5)
    pts[11] = (0.5, 0.5, -np.inf)
    qs = np.concatenate([R.random_cloud(200, 52), (rng.random((200, 3)) * 0.03 + 0.49).astype(np.float32)]).astype(np.float32)
    qs[3] = (np.nan, 0.5, 0.5)
    qs[5] = (0.5, 0.5, np.inf)
    qs[200] = (0.5, -np.inf, np.nan)
    want = _assert_nearest_equal(hip_device, pts, qs, 0.05, (0.05, 0.2, 0.004, None), "a crowded cell")
    assert not np.isin(want[1], [7, 9, 11]).any()
    for k in (3, 5, 200):
        assert want[1][k] == G.NO_INDEX and np.isinf(want[0][k])
    assert (want[1][201:] >= 60).all()
    index = ops.PointIndex(hip_device, pts, cellSize=0.05)
    assert index.info()["indexed"] == pts.shape[0] - 3
    index.destroy()
    # nothing but non-finite points
    _assert_nearest_equal(hip_device, pts[[7, 9, 11]], qs[:10], 0.05, (0.05, None), "no finite point")


def test_nearest_records_and_replays(hip_device):
    dev = hip_device
    pts, qs = R.random_cloud(3000, 21), R.random_cloud(3000, 22)
    want = G.nearest(pts, qs, 0.09)
    index = ops.PointIndex(dev, pts, cellSize=0.05)
    lazy = ops.PointIndex(dev, pts)
    small = ops.PointIndex(dev, pts[:10], cellSize=0.05)
    qbuf = dev.bufferFrom(qs)
    d2, idx, pairs = dev.createBuffer(4 * 3000), dev.createBuffer(4 * 3000), dev.createBuffer(8)
    try:
        with dev.createCommandEncoder("nearest", record=True) as enc:
            index.nearestInto(enc, qbuf, 3000, 0.09, d2, idx, pairs)
            cmd = enc.finish()
        assert np.all(idx.read(np.uint32) == 0), "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
        dev.synchronize()
        assert_bits_equal(idx.read(np.uint32), want[1], "recorded nearest: index")
        assert_bits_equal(d2.read(np.float32), want[0], "recorded nearest: d2")
        examined = int(pairs.read(np.uint64, count=1)[0])
        assert examined % 2 == 0 and 3000 <= examined // 2 < 3000 * 3000
        cmd.destroy()
        with pytest.raises(_lib.StateError):          # an index without a grid builds it in its first query: not while recording
            with dev.createCommandEncoder("doomed", record=True) as enc:
                lazy.nearestInto(enc, qbuf, 3000, 0.09, d2, idx)
        with pytest.raises(_lib.StateError):          # more queries than the room reserved: not while recording
            with dev.createCommandEncoder("doomed", record=True) as enc:
                small.nearestInto(enc, qbuf, 3000, 0.09, d2, idx)
        dev.synchronize()
        small.reserveQueries(3000)
        with dev.createCommandEncoder("reserved", record=True) as enc:
            small.nearestInto(enc, qbuf, 3000, 0.09, d2, idx)
            cmd = enc.finish()
        dev.queue.submit([cmd])
        dev.synchronize()
        assert_bits_equal(idx.read(np.uint32), G.nearest(pts[:10], qs, 0.09)[1], "recorded nearest after reserveQueries")
        cmd.destroy()
    finally:
        for i in (index, lazy, small):
            i.destroy()


# ---------------------------------------------------------------- 3. statistics and metrics
@pytest.mark.parametrize("cutoff", CLOUD_CUTOFFS)
def test_distance_stats_match_the_restatement(hip_device, cutoff):
    dev = hip_device
    pts, qs = R.random_cloud(3000, 21), R.random_cloud(3000, 22)
    d2, _ = G.nearest(pts, qs, cutoff)
    for threshold in (cutoff, 0.6 * cutoff):
        got = ops.pointDistanceStats(dev, d2, cutoff, threshold)
        want = G.distance_stats(d2, cutoff, threshold)
        assert (got["n_found"], got["n_within"], got["sum_q"]) == want, f"cutoff {cutoff}, threshold {threshold}"
        assert got["n"] == 3000 and got["mean"] == want[2] * float(np.float32(cutoff)) / 2.0 ** 24 / want[0]
    assert ops.pointDistanceStats(dev, np.zeros(0, np.float32), 1.0, 0.5) == dict(n=0, n_found=0, n_within=0, sum_q=0, mean=pytest.approx(float("nan"), nan_ok=True))
    for max_distance, threshold in ((1.0, 0.0), (1.0, 1.5), (0.0, 0.0), (float("inf"), 1.0), (1.0, float("nan")), (float("nan"), 1.0), (1.0, -0.5)):
        with pytest.raises(_lib.WdgsError) as e:
            ops.pointDistanceStats(dev, d2, max_distance, threshold)
        assert e.value.code == _lib.WDGS_E_INVALID, (max_distance, threshold)
    _same_metrics(ops.geometryMetrics(dev, qs, pts, cutoff, 0.6 * cutoff), G.geometry_metrics(qs, pts, cutoff, 0.6 * cutoff), f"cloud metrics, cutoff {cutoff}")


def test_metrics_on_two_sampled_planes_and_identical_sets(hip_device):
    dev = hip_device
    a, b, h = R.two_planes()
    delta = R.PLANE_DELTA
    upper = float(np.sqrt(delta ** 2 + h ** 2))
    max_distance = 4 * upper
    for threshold in (upper * 1.001, delta * 0.999):
        got = ops.geometryMetrics(dev, a, b, max_distance, threshold)
        _same_metrics(got, G.geometry_metrics(a, b, max_distance, threshold), f"two planes, threshold {threshold}")
        want_pr = 1.0 if threshold > upper else 0.0
        assert got["precision"] == want_pr and got["recall"] == want_pr and got["fscore"] == want_pr
        assert delta * (1 - 1e-6) <= got["accuracy"] <= upper * (1 + 1e-6) and delta * (1 - 1e-6) <= got["completeness"] <= upper * (1 + 1e-6)
    got = ops.geometryMetrics(dev, a, b, delta * 0.5, delta * 0.25)
    _same_metrics(got, G.geometry_metrics(a, b, delta * 0.5, delta * 0.25), "two planes beyond the cutoff")
    assert np.isnan(got["accuracy"]) and got["outliers_points"] == a.shape[0] and got["fscore"] == 0.0
    got = ops.geometryMetrics(dev, a, a, 0.1, 0.01)
    _same_metrics(got, G.geometry_metrics(a, a, 0.1, 0.01), "identical sets")
    assert got["accuracy"] == 0.0 and got["chamfer"] == 0.0 and got["fscore"] == 1.0
    # device buffers serve as well as arrays; an empty side gives nan, not an error
    got = ops.geometryMetrics(dev, dev.bufferFrom(a), dev.bufferFrom(b), max_distance, upper * 1.001)
    _same_metrics(got, G.geometry_metrics(a, b, max_distance, upper * 1.001), "two planes as device buffers")
    got = ops.geometryMetrics(dev, np.zeros((0, 3), np.float32), b, max_distance, upper)
    assert np.isnan(got["accuracy"]) and np.isnan(got["completeness"]) and got["n_points"] == 0 and got["outliers_reference"] == b.shape[0]


# ---------------------------------------------------------------- 4. the Trainer surface
def test_trainer_evaluate_geometry(hip_device, tmp_path):
    """The smallest synthetic scene (the TSDF tests'): a volume of Gaussians in a frustum.  It has no surface of its own to compare with, so the reference is
    an analytic one inside its box -- the plane z = 5 over the box's x and y -- and the cutoff is wide enough for every mesh to reach it."""
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    rv = np.array([[lo[0], lo[1], 5], [hi[0], lo[1], 5], [hi[0], hi[1], 5], [lo[0], hi[1], 5]], np.float32)
    reference = G.sample_mesh(rv, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), 100.0, 1)["points"]
    path = str(tmp_path / "reference.ply")
    loaders.savePointsPLY(path, reference)
    out = []
    for evaluating in (False, True):
        t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
        try:
            for i in range(6):
                t.step()
                if evaluating and i in (2, 4):
                    iteration, rng_state = t.iteration, t._rng.getstate()
                    before = t.evaluate([0], split="train")
                    r = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5)
                    assert t.iteration == iteration and t._rng.getstate() == rng_state
                    after = t.evaluate([0], split="train")
                    assert before["sse"] == after["sse"] and before["ssim"] == after["ssim"], "evaluate() returns what it returned before"
                    assert r["vertices"] > 0 and r["faces"] > 0 and r["samples"] > 0 and r["n_points"] == r["samples"] and r["n_reference"] == reference.shape[0]
                    assert np.isfinite(r["accuracy"]) and np.isfinite(r["completeness"]) and r["chamfer"] == (r["accuracy"] + r["completeness"]) / 2
                    assert 0.0 <= r["precision"] <= 1.0 and 0.0 <= r["recall"] <= 1.0 and r["ms"] > 0
                    # the pieces by hand give the same numbers; so does the reference read from a file
                    mesh = t.extractMesh(lo, hi, voxel)
                    samples = ops.sampleMesh(dev, mesh, 1.0 / (voxel / 2) ** 2, 0)["points"]
                    assert samples.shape[0] == r["samples"] and mesh["faces"].shape[0] == r["faces"]
                    hand = ops.geometryMetrics(dev, samples, reference, 8.0, 0.5)
                    _same_metrics({k: r[k] for k in hand}, hand, "evaluateGeometry vs the ops by hand")
                    again = t.evaluateGeometry(path, lo, hi, voxel, maxDistance=8.0, threshold=0.5)
                    _same_metrics({k: again[k] for k in hand}, hand, "evaluateGeometry with a PLY path")
                    sparse = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, density=10.0, seed=3)
                    assert 0 < sparse["samples"] < r["samples"]
            t.drain()
            st = t.optimizer.getStateBuffers()
            out.append(dict(g=t.pointCloud.gaussian_3d_buffer.read(np.uint32), sh=t.pointCloud.sh_buffer.read(np.uint32), **{k: st[k].read(np.uint32) for k in st}))
        finally:
            t.destroy()
    for k in out[0]:
        assert_bits_equal(out[1][k], out[0][k], f"evaluating geometry vs not: {k}")
