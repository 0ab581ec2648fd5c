"""CPU: the float32 restatement of the mesh accuracy metrics (tests/geometry_ref.py) against float64 and against what the scheme promises: samples inside
their triangles, totals and uniformity of the pinned hash, degenerate faces, the nearest search against a float64 brute force, and the metrics on two
sampled planes.  The GPU tests (tests/test_gpu_geometry.py) then compare the kernels with the restatement byte for byte and reuse the cases built here."""
import functools

import numpy as np
import pytest

import geometry_ref as G
from harness import assert_bits_equal
from webdgs_amd import loaders

EPS = 2.0 ** -23


# ---------------------------------------------------------------- shared cases (built once, never modified)
@functools.lru_cache(maxsize=None)
def square_samples(n, seed, density=20000.0):
    v, f = G.square_mesh(n)
    s = G.sample_mesh(v, f, density, seed)
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v, f, s


@functools.lru_cache(maxsize=None)
def random_cloud(count, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    a = (rng.random((count, 3)) * scale).astype(np.float32)
    a.setflags(write=False)
    return a


PLANE_DELTA = 0.05


@functools.lru_cache(maxsize=None)
def two_planes():
    """Two parallel unit squares PLANE_DELTA apart, sampled with different seeds, and the covering radius h of each sample set on its square (measured on the
    float32 samples themselves, on a fine lattice of the square, plus the lattice's own half diagonal)."""
    va, fa = G.square_mesh(4, z=0.0)
    vb, fb = G.square_mesh(3, z=PLANE_DELTA)
    a = G.sample_mesh(va, fa, 1500.0, 11)["points"]
    b = G.sample_mesh(vb, fb, 1500.0, 12)["points"]
    m = 96
    g = (np.arange(m) + 0.5) / m
    lattice = np.stack([np.repeat(g, m), np.tile(g, m)], axis=1)
    h = 0.0
    for s in (a, b):
        s64 = s[:, :2].astype(np.float64)
        d2 = np.concatenate([((lattice[i:i + 1024, None, :] - s64[None, :, :]) ** 2).sum(axis=2).min(axis=1) for i in range(0, lattice.shape[0], 1024)])
        h = max(h, float(np.sqrt(d2.max())) + np.sqrt(2.0) * 0.5 / m)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, h


# ---------------------------------------------------------------- 1. sampling
def test_hash_and_unit_are_the_pinned_functions():
    # mix is the "lowbias32" finaliser: fixed values, computed by hand from the definition in Python integers
    def mix_py(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x

    def h_py(seed, t, k, j):
        return mix_py(mix_py((mix_py(mix_py((seed + 0x9E3779B9) & 0xFFFFFFFF) ^ t) + k) & 0xFFFFFFFF) ^ ((j * 0x85EBCA6B + 1) & 0xFFFFFFFF))

    for args in ((0, 0, 0, 0), (5, 7, 0xFFFFFFFF, 0), (0xFFFFFFFF, 123456, 99, 2), (1, 0xFFFFFFFE, 0x80000000, 1)):
        assert int(G.sample_hash(*args)[0]) == h_py(*args)
    u = G.unit(np.array([0, 0xFFFFFFFF, 1 << 9], np.uint32))
    assert u.dtype == np.float32 and u[0] == np.float32(2.0 ** -24) and u[1] == np.float32(1.0 - 2.0 ** -24) and u[2] == np.float32(1.5 * 2.0 ** -23)


@pytest.mark.parametrize("n,seed", [(16, 1), (16, 7), (32, 3), (4, 5)])
def test_points_lie_in_their_triangles_and_totals_follow_the_area(n, seed):
    v, f, s = square_samples(n, seed)
    F = f.shape[0]
    assert F == 2 * n * n and s["total"] == s["points"].shape[0] == int(s["counts"].sum())
    print(f"unit square n={n} seed={seed}: total {s['total']}, |total - 20000| = {abs(s['total'] - 20000)}, bound {2 * np.sqrt(F):.1f}")
    assert abs(s["total"] - 20000.0) <= 2.0 * np.sqrt(F)      # four standard deviations of F independent dithers of variance <= 1/4
    u, w, residual = G.barycentric64(s["points"], v, f, s["face"])
    tol = 8 * EPS
    assert u.min() >= -tol and w.min() >= -tol and (u + w).max() <= 1 + tol
    assert residual.max() <= tol * float(np.abs(v).max())
    # samples of a triangle are consecutive, triangles in order
    assert np.all(np.diff(s["face"].astype(np.int64)) >= 0)
    assert np.array_equal(np.bincount(s["face"], minlength=F), s["counts"])


def test_tilted_triangles_keep_their_samples_in_plane():
    rng = np.random.default_rng(2)
    v = (rng.random((40, 3)) * 6 - 3).astype(np.float32)
    f = rng.integers(0, 40, (60, 3)).astype(np.uint32)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    s = G.sample_mesh(v, f, 30.0, 9)
    assert s["total"] > 2000
    u, w, residual = G.barycentric64(s["points"], v, f, s["face"])
    # per-axis error of (A + u e1) + v e2 is a few ulps of the largest coordinate; in barycentric units it is divided by the triangle's height, so the
    # barycentric test is made on the unit square above (heights >= 1/32) and the residual here, against the coordinates' size
    assert residual.max() <= 8 * EPS * float(np.abs(v).max())
    assert u.min() >= -1e-4 and w.min() >= -1e-4 and (u + w).max() <= 1 + 1e-4


def test_uniformity_chi_square():
    v, f, s = square_samples(4, 5)
    p = s["points"]
    hist, _, _ = np.histogram2d(p[:, 0], p[:, 1], bins=8, range=[[0, 1], [0, 1]])
    expect = s["total"] / 64.0
    chi2 = float(((hist - expect) ** 2 / expect).sum())
    print(f"chi^2 of the 8x8 histogram, n=4 seed=5: {chi2:.1f} (99.9 % point at 63 degrees of freedom: 103.4)")
    assert chi2 < 103.4


def test_degenerate_and_out_of_range_faces_get_no_samples():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 5], [0, 0, 0], [0, 1, 4], [2, 1, 0]], np.uint32)   # fine, collinear, vertex 5 >= V, a point, a NaN corner, fine
    for seed in range(8):
        c = G.sample_counts(v, f, 1000.0, seed)
        assert c[1] == 0 and c[2] == 0 and c[3] == 0 and c[4] == 0, c
        assert 499 <= c[0] <= 501 and 499 <= c[5] <= 501
    s = G.sample_mesh(v, f, 1000.0, 3)
    assert set(np.unique(s["face"])) == {0, 5}
    assert G.sample_mesh(v, np.zeros((0, 3), np.uint32), 10.0)["total"] == 0
    assert G.sample_counts(v, f, 1e38, 0)[0] == 2 ** 31 - 1 and G.sample_counts(v, f, 3e38, 0)[0] == 2 ** 31 - 1
    with pytest.raises(OverflowError):
        G.sample_mesh(v, f, 5e9)


def test_sampling_is_a_function_of_its_inputs():
    v, f = G.square_mesh(4)
    a, b, c = G.sample_mesh(v, f, 500.0, 1), G.sample_mesh(v, f, 500.0, 1), G.sample_mesh(v, f, 500.0, 2)
    assert a["points"].tobytes() == b["points"].tobytes() and a["points"].tobytes() != c["points"].tobytes()


# ---------------------------------------------------------------- 2. nearest
@pytest.mark.parametrize("cutoff", [0.02, 0.09])
def test_float32_brute_force_agrees_with_float64(cutoff):
    pts, qs = random_cloud(3000, 21), random_cloud(3000, 22)
    d2, idx = G.nearest(pts, qs, cutoff)
    best, bidx, second = G.nearest64(pts, qs)
    r2 = float(np.float32(cutoff)) ** 2
    margin = 8 * EPS * r2
    # decided: the best is clearly apart from the second best, and clearly on one side of the cutoff (|d2 - r2| beyond the roundings of both)
    decided = (second - best > margin) & (np.abs(best - r2) > 8 * EPS * np.maximum(best, r2))
    assert decided.mean() > 0.99
    inside = decided & (best < r2)
    outside = decided & (best > r2)
    assert inside.any() and outside.any()
    assert np.array_equal(idx[inside].astype(np.int64), bidx[inside])
    assert np.all(np.abs(d2[inside].astype(np.float64) - best[inside]) <= 8 * EPS * best[inside] + 1e-12)
    assert np.all(idx[outside] == G.NO_INDEX) and np.all(np.isinf(d2[outside]))


def test_ties_non_finite_values_and_empty_sets():
    pts = np.zeros((300, 3), np.float32) + np.float32(0.25)
    d2, idx = G.nearest(pts, np.array([[0.25, 0.25, 0.5]], np.float32), 1.0)
    assert idx[0] == 0 and d2[0] == np.float32(0.0625)
    # an exact tie between two different points: the lower index, wherever it sits
    pts = np.array([[1, 0, 0], [-1, 0, 0], [0, 3, 0]], np.float32)
    assert G.nearest(pts, np.zeros((1, 3), np.float32), 2.0)[1][0] == 0 and G.nearest(pts[::-1].copy(), np.zeros((1, 3), np.float32), 2.0)[1][0] == 1
    # d2 == r2 is a candidate; just beyond is not
    assert G.nearest(pts, np.zeros((1, 3), np.float32), 1.0)[1][0] == 0 and G.nearest(pts, np.zeros((1, 3), np.float32), 0.99)[1][0] == G.NO_INDEX
    pts = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0.5, 0, 0]], np.float32)
    qs = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0]], np.float32)
    d2, idx = G.nearest(pts, qs, 1.0)
    assert idx.tolist() == [2, G.NO_INDEX, G.NO_INDEX, G.NO_INDEX] and d2[0] == np.float32(0.25) and np.all(np.isinf(d2[1:]))
    d2, idx = G.nearest(np.zeros((0, 3), np.float32), qs, 1.0)
    assert np.all(np.isinf(d2)) and np.all(idx == G.NO_INDEX)
    assert G.nearest(pts, np.zeros((0, 3), np.float32), 1.0)[0].shape == (0,)


# ---------------------------------------------------------------- 3. statistics and metrics
def test_distance_stats_by_hand():
    d2 = np.array([0.0, 0.25, 1.0, np.inf, 0.0625, np.inf], np.float32)
    n_found, n_within, sum_q = G.distance_stats(d2, 1.0, 0.5)
    assert (n_found, n_within) == (4, 3)
    assert sum_q == 0 + (1 << 23) + (1 << 24) + (1 << 22)
    assert G.distance_stats(np.zeros(0, np.float32), 1.0, 0.5) == (0, 0, 0)


def test_two_sampled_planes():
    a, b, h = two_planes()
    delta = PLANE_DELTA
    upper = float(np.sqrt(delta ** 2 + h ** 2))
    max_distance = 4 * upper
    d2_ab, _ = G.nearest(b, a, max_distance)
    d2_ba, _ = G.nearest(a, b, max_distance)
    d_all = np.sqrt(np.concatenate([d2_ab, d2_ba]).astype(np.float64))
    slack = 8 * EPS
    print(f"two planes {delta} apart: covering radius {h:.4f}, distances in [{d_all.min():.5f}, {d_all.max():.5f}], bounds [{delta}, {upper:.5f}]")
    assert d_all.min() >= delta * (1 - slack) and d_all.max() <= upper * (1 + slack)
    m = G.geometry_metrics(a, b, max_distance, upper * 1.001)
    assert m["precision"] == 1.0 and m["recall"] == 1.0 and m["fscore"] == 1.0 and m["outliers_points"] == 0 and m["outliers_reference"] == 0
    q = max_distance / 2.0 ** 24                      # each distance is truncated to a multiple of q
    assert delta * (1 - slack) - q <= m["accuracy"] <= upper * (1 + slack) and delta * (1 - slack) - q <= m["completeness"] <= upper * (1 + slack)
    assert m["chamfer"] == (m["accuracy"] + m["completeness"]) / 2
    m = G.geometry_metrics(a, b, max_distance, delta * 0.999)
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["fscore"] == 0.0
    # a cutoff below the gap: everything is an outlier, the means are undefined
    m = G.geometry_metrics(a, b, delta * 0.5, delta * 0.25)
    assert m["outliers_points"] == a.shape[0] and m["outliers_reference"] == b.shape[0] and np.isnan(m["accuracy"]) and np.isnan(m["chamfer"]) and m["fscore"] == 0.0


def test_identical_sets():
    a, _, _ = two_planes()
    m = G.geometry_metrics(a, a, 0.1, 0.01)
    assert m["accuracy"] == 0.0 and m["completeness"] == 0.0 and m["chamfer"] == 0.0
    assert m["precision"] == 1.0 and m["recall"] == 1.0 and m["fscore"] == 1.0 and m["n_points"] == m["n_reference"] == a.shape[0]


# ---------------------------------------------------------------- 4. point-set files
def test_points_ply_round_trip(tmp_path):
    pts = random_cloud(777, 61).copy()
    pts[5] = (np.nan, -0.0, np.inf)
    path = str(tmp_path / "points.ply")
    loaders.savePointsPLY(path, pts)
    assert_bits_equal(loaders.loadPointsPLY(path), pts, "points PLY")
    loaders.savePointsPLY(path, np.zeros((0, 3), np.float32))
    assert loaders.loadPointsPLY(path).shape == (0, 3)
    # a mesh PLY with colours: the positions, other properties skipped
    v, f = G.square_mesh(3)
    loaders.saveMeshPLY(path, dict(vertices=v, faces=f, colours=np.full((v.shape[0], 3), 7, np.uint8)))
    assert_bits_equal(loaders.loadPointsPLY(path), v, "a mesh PLY's vertices")
    with pytest.raises(ValueError):
        loaders.savePointsPLY(path, np.zeros((4, 2), np.float32))
