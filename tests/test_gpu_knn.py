"""GPU: the k-nearest query of the point index and the neighbour-based scale initialisation (csrc/geometry.hip) against the float32
restatement (tests/knn_ref.py), byte for byte: both sides of every list capacity, ties cut by k, cell-size independence, k = 1 against ``nearest``,
self-exclusion, few points, the early exit's pair counts, refusals, recording, and the scales written into a loaded cloud."""
import ctypes

import numpy as np
import pytest

from webdgs_amd import _lib, ops

import geometry_ref as G
import knn_ref as KR
import test_knn_reference as R
from harness import assert_bits_equal

pytestmark = pytest.mark.gpu

NO = KR.NO_INDEX
MARK = 0x7FC01234


def _assert_rows_equal(got, want, k, what):
    assert got["d2"].shape == got["index"].shape == (want[0].shape[0], k), what
    assert_bits_equal(got["index"], np.ascontiguousarray(want[1][:, :k]), f"{what}: index")
    assert_bits_equal(got["d2"], np.ascontiguousarray(want[0][:, :k]), f"{what}: d2")


def _pairs_of(dev, index, qbuf, count, k, cutoff, exclude_self):
    d2, idx, pairs = dev.createBuffer(4 * count * k), dev.createBuffer(4 * count * k), dev.createBuffer(8)
    try:
        pairs.clear()
        index.kNearestInto(None, qbuf, count, k, cutoff, d2, idx, exclude_self, pairs)
        dev.synchronize()
        return int(pairs.read(np.uint64, count=1)[0]), d2.read(np.float32, count=count * k).reshape(count, k), idx.read(np.uint32, count=count * k).reshape(count, k)
    finally:
        for b in (d2, idx, pairs):
            b.destroy()


# ---------------------------------------------------------------- 1. random
@pytest.mark.parametrize("cutoff", R.RANDOM_CUTOFFS)
def test_random_cloud_every_capacity(hip_device, cutoff):
    pts, qs = R.random_case()
    want = R.random_reference(cutoff)
    index = ops.PointIndex(hip_device, pts, cellSize=min(cutoff, 0.07))
    try:
        for k in R.RANDOM_KS:
            _assert_rows_equal(index.kNearest(qs, k, cutoff), want, k, f"3000 x 1000, cutoff {cutoff}, k = {k}")
    finally:
        index.destroy()
    found = (want[1] != NO).sum(axis=1)
    if cutoff == 0.05:
        assert (found < 3).mean() > 0.3
    if cutoff == 4.0:
        assert (found == 16).sum() == 996


# ---------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("k", (3, 8))
def test_lattice_ties_cut_by_k(hip_device, k):
    pts, qs = R.lattice_case()
    want = KR.k_nearest(pts, qs, k, 1.0)
    for row in (0, 17, 124):
        corners = np.sort(np.flatnonzero(np.all(np.abs(pts - qs[row]) == 0.5, axis=1)))
        assert want[1][row].tolist() == corners[:k].tolist()
    exact = KR.k_nearest(pts, qs[125:250], k, 0.5)          # the second candidate at d2 = r2 exactly; for k = 3 the third slot is padding
    assert np.all(exact[0][:, 1] == np.float32(0.25)) and np.all(exact[1][:, 2] == NO)
    for cell in (1.0, 0.5, 0.3, 0.37, 2.0):
        index = ops.PointIndex(hip_device, pts, cellSize=cell)
        try:
            _assert_rows_equal(index.kNearest(qs, k, 1.0), want, k, f"lattice, k = {k}, cell edge {cell}")
            _assert_rows_equal(index.kNearest(qs[125:250], k, 0.5), exact, k, f"lattice, d2 = r2, k = {k}, cell edge {cell}")
        finally:
            index.destroy()


def test_kth_candidate_exactly_on_the_cutoff(hip_device):
    """Edge midpoints with the cutoff at 0.5: the two end points sit at d2 = r2 = 0.25.  With k = 2 the k-th candidate is exactly on the cutoff."""
    pts, qs = R.lattice_case()
    want = KR.k_nearest(pts, qs[125:250], 2, 0.5)
    assert np.all(want[0] == np.float32(0.25)) and np.all(want[1] != NO)
    for cell in (1.0, 0.3, None):
        index = ops.PointIndex(hip_device, pts, cellSize=cell)
        try:
            _assert_rows_equal(index.kNearest(qs[125:250], 2, 0.5), want, 2, f"d2 = r2 for the k-th, cell edge {cell}")
        finally:
            index.destroy()


# ---------------------------------------------------------------- 3. cell edge
def test_cell_size_independence(hip_device):
    pts, qs = R.random_case()
    r, k = 0.3, 5
    want = R.random_reference(r)
    for cell in (r, 2.7 * r, r / 3, None, 1e-9, 50.0):
        index = ops.PointIndex(hip_device, pts, cellSize=cell)
        try:
            _assert_rows_equal(index.kNearest(qs, k, r), want, k, f"cell edge {cell} (grid {index.info()['dims']})")
        finally:
            index.destroy()


# ---------------------------------------------------------------- 4. k = 1 against nearest
@pytest.mark.parametrize("cutoff", (0.05, 0.3))
def test_k1_is_nearest_bytes_and_pairs(hip_device, cutoff):
    dev = hip_device
    pts, qs = R.random_case()
    n = qs.shape[0]
    index = ops.PointIndex(dev, pts, cellSize=0.04)
    qbuf = dev.bufferFrom(qs)
    d2, idx, pairs = dev.createBuffer(4 * n), dev.createBuffer(4 * n), dev.createBuffer(8)
    try:
        pairs.clear()
        index.nearestInto(None, qbuf, n, cutoff, d2, idx, pairs)
        dev.synchronize()
        near = (d2.read(np.float32, count=n), idx.read(np.uint32, count=n), int(pairs.read(np.uint64, count=1)[0]))
        got_pairs, got_d2, got_idx = _pairs_of(dev, index, qbuf, n, 1, cutoff, False)
        assert_bits_equal(got_idx[:, 0], near[1], "k = 1: index")
        assert_bits_equal(got_d2[:, 0], near[0], "k = 1: d2")
        assert got_pairs == near[2] > 0
        want = G.nearest(pts, qs, cutoff)
        assert_bits_equal(near[1], want[1], "nearest: index")
    finally:
        for b in (qbuf, d2, idx, pairs):
            b.destroy()
        index.destroy()


# ---------------------------------------------------------------- 5. self-exclusion
def test_self_exclusion_among_duplicates(hip_device):
    pts, twin_of = R.duplicates_case()
    copies = 1800 + np.arange(200)
    index = ops.PointIndex(hip_device, pts)
    try:
        for k in (3, 4):
            got = index.kNearest(pts, k, 4.0, excludeSelf=True)
            _assert_rows_equal(got, KR.k_nearest(pts, pts, k, 4.0, exclude_self=True), k, f"self-query with the flag, k = {k}")
            assert not np.any(got["index"] == np.arange(2000, dtype=np.uint32)[:, None])
            assert np.all(got["d2"][copies, 0] == 0) and np.array_equal(got["index"][copies, 0], twin_of.astype(np.uint32))
            assert np.all(got["d2"][twin_of, 0] == 0) and np.array_equal(got["index"][twin_of, 0], copies.astype(np.uint32))
        got = index.kNearest(pts, 3, 4.0)
        _assert_rows_equal(got, KR.k_nearest(pts, pts, 3, 4.0), 3, "self-query without the flag")
        assert np.array_equal(got["index"][copies, 0], twin_of.astype(np.uint32)) and np.array_equal(got["index"][twin_of, 0], twin_of.astype(np.uint32))
        assert np.all(got["d2"][:, 0] == 0)
    finally:
        index.destroy()


# ---------------------------------------------------------------- 6. few points
def test_few_points(hip_device):
    dev = hip_device
    qs = R.cloud_with_bad_rows(70, 31, (4,))
    cases = [("M = 0", np.zeros((0, 3), np.float32), qs, 3, False),
             ("M = 1 with the flag", qs[:1], qs[:1], 3, True),
             ("M = 2, k = 3", qs[:2], qs, 3, False),
             ("M = 2, k = 3, self", qs[:2], qs[:2], 3, True),
             ("no finite point", np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32), qs, 5, False)]
    for what, pts, queries, k, flag in cases:
        want = KR.k_nearest(pts, queries, k, 2.0, exclude_self=flag)
        for cell in (0.5, None):
            index = ops.PointIndex(dev, pts, cellSize=cell)
            try:
                _assert_rows_equal(index.kNearest(queries, k, 2.0, excludeSelf=flag), want, k, f"{what}, cell edge {cell}")
            finally:
                index.destroy()
    assert np.all(KR.k_nearest(qs[:1], qs[:1], 3, 2.0, exclude_self=True)[1] == NO)
    index = ops.PointIndex(dev, qs, cellSize=0.3)
    try:
        empty = index.kNearest(np.zeros((0, 3), np.float32), 3, 1.0)
        assert empty["d2"].shape == (0, 3) and empty["index"].shape == (0, 3)
    finally:
        index.destroy()


# ---------------------------------------------------------------- 7. the early exit works
def test_early_exit_pair_count_does_not_depend_on_a_wide_cutoff(hip_device):
    """Self-query with the flag of the 16^3 integer lattice, cell edge 1, k = 3: every point's third neighbour is at d2 = 1 and T_2^2 is about 4, so the search
    ends after ring 2 at the latest inside either box, and the pairs examined are the same for a cutoff of 3 and of twice the extent."""
    dev = hip_device
    g = np.arange(16, dtype=np.float32)
    pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    index = ops.PointIndex(dev, pts, cellSize=1.0)
    qbuf = dev.bufferFrom(pts)
    try:
        wide = _pairs_of(dev, index, qbuf, 4096, 3, 30.0, True)
        tight = _pairs_of(dev, index, qbuf, 4096, 3, 3.0, True)
        assert wide[0] == tight[0] > 0
        assert wide[0] <= 4096 * 125, "no query looks beyond ring 2"
        assert_bits_equal(wide[2], tight[2], "index")
        assert np.all(wide[1] == 1.0)
        want = KR.k_nearest(pts, pts, 3, 3.0, exclude_self=True)
        assert_bits_equal(tight[2], want[1], "lattice self-query: index")
    finally:
        qbuf.destroy()
        index.destroy()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_write_nothing(hip_device):
    dev = hip_device
    pts, qs = R.random_case()
    n = 100
    index = ops.PointIndex(dev, pts, cellSize=0.1)
    qbuf = dev.bufferFrom(qs[:n])
    d2, idx = dev.createBuffer(4 * n * 17), dev.createBuffer(4 * n * 17)
    marker = np.full(n * 17, MARK, np.uint32)
    d2.write(marker)
    idx.write(marker)
    try:
        for k, cutoff in ((0, 0.1), (17, 0.1), (3, 0.0), (3, -1.0), (3, float("inf")), (3, float("nan"))):
            with pytest.raises(_lib.WdgsError) as e:
                index.kNearestInto(None, qbuf, n, k, cutoff, d2, idx)
            assert e.value.code == _lib.WDGS_E_INVALID, (k, cutoff)
        for flags in (2, 3, 0x80000000):
            with pytest.raises(_lib.WdgsError) as e:
                _lib.check(dev.lib.wdgs_point_index_k_nearest(index.handle, qbuf.ptr, n, 3, 0.1, flags, d2.ptr, idx.ptr, None))
            assert e.value.code == _lib.WDGS_E_INVALID, flags
        dev.synchronize()
        assert_bits_equal(d2.read(np.uint32), marker, "a refused query writes nothing: d2")
        assert_bits_equal(idx.read(np.uint32), marker, "a refused query writes nothing: index")
        small = dev.createBuffer(4 * n * 3 - 4)
        with pytest.raises(ValueError):
            index.kNearestInto(None, qbuf, n, 3, 0.1, small, idx)
        with pytest.raises(ValueError):
            index.kNearestInto(None, qbuf, n, 3, 0.1, d2, small)
        with pytest.raises(ValueError):
            index.kNearestInto(None, qbuf, n + 1, 3, 0.1, d2, idx)
        with pytest.raises(ValueError):
            index.kNearestInto(None, qbuf, n, 3, 0.1, d2, idx, pairs=dev.createBuffer(4))
        # the scales' own refusals
        g = dev.createBuffer(24 * n)
        for k, min_d2 in ((3, 0.0), (3, -1e-7), (3, float("inf")), (3, float("nan")), (0, 1e-7), (17, 1e-7)):
            with pytest.raises(_lib.WdgsError) as e:
                _lib.check(dev.lib.wdgs_point_cloud_neighbour_scales(dev.handle, g.ptr, n, d2.ptr, k, min_d2, None))
            assert e.value.code == _lib.WDGS_E_INVALID, (k, min_d2)
    finally:
        index.destroy()


# ---------------------------------------------------------------- 9. recording
def test_k_nearest_records_and_replays(hip_device):
    dev = hip_device
    pts, qs = R.random_case()
    n, k, cutoff = qs.shape[0], 5, 0.3
    want = R.random_reference(cutoff)
    index = ops.PointIndex(dev, pts[:10], cellSize=0.05)           # room for 10 queries only
    full = ops.PointIndex(dev, pts, cellSize=0.05)
    qbuf = dev.bufferFrom(qs)
    d2, idx = dev.createBuffer(4 * n * k), dev.createBuffer(4 * n * k)
    try:
        eager = full.kNearest(qs, k, cutoff)
        _assert_rows_equal(eager, want, k, "eager")
        idx.clear()
        with dev.createCommandEncoder("kNearest", record=True) as enc:
            full.kNearestInto(enc, qbuf, n, k, cutoff, d2, idx, True)
            cmd = enc.finish()
        assert np.all(idx.read(np.uint32) == 0), "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
        dev.synchronize()
        flagged = KR.k_nearest(pts, qs, k, cutoff, exclude_self=True)
        assert_bits_equal(idx.read(np.uint32).reshape(n, k), flagged[1], "recorded kNearest: index")
        assert_bits_equal(d2.read(np.float32).reshape(n, k), flagged[0], "recorded kNearest: d2")
        cmd.destroy()
        with pytest.raises(_lib.StateError):                       # more queries than the room reserved: not while recording
            with dev.createCommandEncoder("doomed", record=True) as enc:
                index.kNearestInto(enc, qbuf, n, k, cutoff, d2, idx)
        dev.synchronize()
        index.reserveQueries(n)
        with dev.createCommandEncoder("reserved", record=True) as enc:
            index.kNearestInto(enc, qbuf, n, k, cutoff, d2, idx)
            cmd = enc.finish()
        for _ in range(2):
            dev.queue.submit([cmd])
        dev.synchronize()
        small = KR.k_nearest(pts[:10], qs, k, cutoff)
        assert_bits_equal(idx.read(np.uint32).reshape(n, k), small[1], "recorded after reserveQueries: index")
        assert_bits_equal(d2.read(np.float32).reshape(n, k), small[0], "recorded after reserveQueries: d2")
        cmd.destroy()
    finally:
        for i in (index, full):
            i.destroy()


# ---------------------------------------------------------------- 10. scales
def test_scales_from_neighbours(hip_device, orc):
    dev = hip_device
    data = R.scales_case()
    n = data.num_points
    pos = KR.unpack_positions(data.gaussians)
    outliers, quads = list(R.SCALES_OUTLIERS), np.array(R.SCALES_QUADS)
    minus_five = np.float16(-5.0).view(np.uint16)

    def run(max_distance):
        pc = ops.createPointCloud(dev, data.gaussians, data.sh, data.sh_deg)
        sh_before = pc.sh_buffer.read(np.uint32)
        out = ops.initScalesFromNeighbours(dev, pc, k=3, maxDistance=max_distance)
        assert_bits_equal(pc.sh_buffer.read(np.uint32), sh_before, "the sh buffer is untouched")
        return pc.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6)[:n], out

    # the default cutoff: twice the widest extent, every other point a candidate
    widest = float((pos.max(axis=0).astype(np.float64) - pos.min(axis=0).astype(np.float64)).max())
    d2, idx = KR.k_nearest(pos, pos, 3, 2.0 * widest, exclude_self=True)
    want_g, want_mean, want_found = KR.neighbour_scales(data.gaussians, d2, 1e-7, orc)
    got_g, out = run(None)
    assert_bits_equal(got_g, want_g, "records after initScalesFromNeighbours")
    assert_bits_equal(out["meanD2"], want_mean, "meanD2")
    assert_bits_equal(out["found"], want_found, "found")
    assert np.all(want_found == 3)
    halves, before = got_g.view(np.uint16).reshape(-1, 12), data.gaussians.view(np.uint16).reshape(-1, 12)
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 11]
    assert_bits_equal(np.ascontiguousarray(halves[:, keep]), np.ascontiguousarray(before[:, keep]), "every other half")
    assert np.all(halves[quads, 8:11] == np.float16(0.5 * np.log(1e-7)).view(np.uint16)), "coincident points get the clamp"
    assert np.all(halves[:, 8:11] != minus_five)
    # a small cutoff: the outliers have no neighbour and keep their record
    d2s, _ = KR.k_nearest(pos, pos, 3, 1.5, exclude_self=True)
    want_g, want_mean, want_found = KR.neighbour_scales(data.gaussians, d2s, 1e-7, orc)
    got_g, out = run(1.5)
    assert_bits_equal(got_g, want_g, "records with a small cutoff")
    assert_bits_equal(out["meanD2"], want_mean, "meanD2 with a small cutoff")
    assert_bits_equal(out["found"], want_found, "found with a small cutoff")
    assert np.all(out["found"][outliers] == 0) and np.all(np.isinf(out["meanD2"][outliers]))
    assert_bits_equal(got_g[outliers], data.gaussians[outliers], "the outliers' records")
    assert np.all(got_g.view(np.uint16).reshape(-1, 12)[outliers, 8:11] == minus_five)
    # the returned numbers are the query's own
    index = ops.PointIndex(dev, pos)
    try:
        q = index.kNearest(pos, 3, 1.5, excludeSelf=True)
    finally:
        index.destroy()
    assert_bits_equal(q["d2"], d2s, "the query by hand")
    assert np.array_equal(out["found"], np.isfinite(q["d2"]).sum(axis=1).astype(np.uint32))
    # the unpacked positions are the records' halves, exactly
    g = dev.bufferFrom(data.gaussians)
    p = dev.createBuffer(12 * n)
    _lib.check(dev.lib.wdgs_point_cloud_positions(dev.handle, g.ptr, n, p.ptr))
    assert_bits_equal(p.read(np.float32, count=3 * n).reshape(n, 3), pos, "positions")
    b = ops.PointIndex(dev, p, count=n)
    try:
        bounds = b.bounds()
    finally:
        b.destroy()
    assert_bits_equal(bounds["lo"], pos.min(axis=0), "bounds lo")
    assert_bits_equal(bounds["hi"], pos.max(axis=0), "bounds hi")
