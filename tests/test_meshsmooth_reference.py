"""No GPU: properties of the restatement of mesh adjacency, Taubin smoothing and vertex normals (tests/meshsmooth_ref.py) -- the rows,
the closed solids' Euler characteristic, invariance under a permutation of the faces, what smoothing does to a noisy sphere, the normals of a clean one --
and the mesh PLY with and without normals."""
import struct

import numpy as np
import pytest

from webdgs_amd import loaders

import meshsmooth_ref as R

SMALL = sorted(n for n in R.CASES if n not in ("many-faces", "random"))


@pytest.mark.parametrize("name", SMALL)
def test_rows_are_ascending_symmetric_and_complete(name):
    m, e = R.case(name), R.expected(name)
    V, F = m["vertices"].shape[0], m["faces"].shape[0]
    rs, nb = e["rowStart"], e["neighbours"]
    assert rs.shape == (V + 1,) and rs[0] == 0 and rs[V] == nb.shape[0] == e["stats"]["directedEdges"] == 2 * e["stats"]["edges"]
    rows = [[int(u) for u in nb[rs[v]:rs[v + 1]]] for v in range(V)]
    for v, row in enumerate(rows):
        assert row == sorted(set(row)) and v not in row, f"{name}: row {v} = {row}"
        for u in row:
            assert v in rows[u], f"{name}: {u} in row({v}) but not the reverse"
    adj = R.adjacency(m["faces"], V)
    assert sum(adj["multiplicity"]) == 6 * (F - e["stats"]["invalidFaces"])
    assert e["stats"]["isolatedVertices"] == sum(1 for r in rows if not r) and e["stats"]["maxDegree"] == max([len(r) for r in rows] or [0])
    for k, n in R.EXPECT.get(name, {}).items():
        assert e["stats"][k] == n, f"{name}: {k} = {e['stats'][k]}"


def test_closed_solids_have_no_boundary_and_euler_characteristic_two():
    ico = R.icosphere(2)
    for name, (v, f) in (("tetrahedron", R.TETRAHEDRON), ("octahedron", R.OCTAHEDRON), ("icosphere", ico)):
        st = R.adjacency(f, len(v))["stats"]
        assert st["boundaryEdges"] == st["nonManifoldEdges"] == st["invalidFaces"] == st["isolatedVertices"] == 0, name
        assert len(v) - st["edges"] + len(f) == 2, name
    assert len(ico[0]) == 162


@pytest.mark.parametrize("name", ["noisy-icosphere", "octahedron", "fin", "grid-pinned", "tile-above", "non-finite"])
def test_a_permutation_of_the_faces_changes_no_smoothed_bit(name):
    m, e = R.case(name), R.expected(name)
    perm = np.random.default_rng(5).permutation(m["faces"].shape[0])
    faces = m["faces"][perm]
    again = R.smooth(m["vertices"], faces, **m["smoothing"])
    assert again.tobytes() == e["smoothed"].tobytes()
    if name in ("noisy-icosphere", "octahedron", "grid-pinned"):   # manifold and consistently oriented: one forward slot per directed edge
        assert R.normals(m["vertices"], faces).tobytes() == e["normals"].tobytes()


def test_the_copy_rules():
    m, e = R.case("overflow"), R.expected("overflow")
    moved = [bool(np.any(e["smoothed"][v] != m["vertices"][v])) for v in range(5)]
    assert moved == [False, True, True, False, False] and np.all(np.isfinite(e["smoothed"]))
    m, e = R.case("non-finite"), R.expected("non-finite")
    bad = ~np.all(np.isfinite(m["vertices"]), axis=1)
    assert bad.sum() == 2 and e["smoothed"][bad].tobytes() == m["vertices"][bad].tobytes()
    assert np.all(np.isfinite(e["smoothed"][~bad])) and np.all(np.any(e["smoothed"][~bad] != m["vertices"][~bad], axis=1))
    m, e = R.case("triangle-pinned"), R.expected("triangle-pinned")
    assert e["smoothed"].tobytes() == m["vertices"].tobytes()
    m, e = R.case("triangle-unpinned"), R.expected("triangle-unpinned")
    assert np.all(np.any(e["smoothed"] != m["vertices"], axis=1))
    m, e = R.case("grid-pinned"), R.expected("grid-pinned")
    edge = e["boundary"] == 1
    assert edge.sum() == 32 and e["smoothed"][edge].tobytes() == m["vertices"][edge].tobytes() and np.any(e["smoothed"][~edge] != m["vertices"][~edge])
    assert R.smooth(m["vertices"], m["faces"], iterations=0).tobytes() == m["vertices"].tobytes()
    assert R.smooth(m["vertices"], m["faces"], iterations=4, lam=0.0, mu=0.0).tobytes() == m["vertices"].tobytes()


def test_taubin_denoises_a_sphere_and_shrinks_it_less_than_laplacian_smoothing():
    v, f = R.noisy_icosphere(seed=7, sigma=0.03)
    adj = R.adjacency(f, v.shape[0])
    radius = lambda p: np.linalg.norm(p.astype(np.float64), axis=1)
    before = radius(np.asarray(v, np.float32))
    taubin = radius(R.smooth(v, f, 10, adj=adj))
    laplace = radius(R.smooth(v, f, 10, mu=0.0, adj=adj))
    print(f"sigma {before.std():.4f} -> {taubin.std():.4f}; mean radius {before.mean():.4f} -> {taubin.mean():.4f} (Taubin), {laplace.mean():.4f} (Laplacian)")
    assert taubin.std() < before.std()
    assert abs(taubin.mean() - before.mean()) < abs(laplace.mean() - before.mean())


def test_normals_of_the_clean_icosphere_point_outward_and_have_unit_length():
    v, f = R.icosphere(2)
    p = np.asarray(v, np.float32)
    n = R.normals(p, f).astype(np.float64)
    assert np.all(np.sum(n * p, axis=1) > 0)
    # n = s / sqrt(q), q = (sx sx + sy sy) + sz sz: a square, and the two sums behind it, put at most three roundings on q, which the root halves; the root
    # and the quotient add one each: |n| = 1 + 3.5 u to first order, u = 2^-24.  4 u leaves room for the second-order terms.
    assert np.max(np.abs(np.linalg.norm(n, axis=1) - 1.0)) <= 4 * 2.0 ** -24
    assert R.normals(R.case("no-faces")["vertices"], np.zeros((0, 3))).tobytes() == np.zeros((5, 3), np.float32).tobytes()


def test_mesh_ply_round_trips_with_normals_and_is_unchanged_without(tmp_path):
    m = R.case("octahedron")
    v, f = m["vertices"], m["faces"]
    n = R.expected("octahedron")["normals"]
    c = np.arange(18, dtype=np.uint8).reshape(6, 3)
    for colours in (None, c):
        plain = dict(vertices=v, faces=f, colours=colours)
        header = ["ply", "format binary_little_endian 1.0", "element vertex 6", "property float x", "property float y", "property float z"]
        header += ["property uchar red", "property uchar green", "property uchar blue"] if colours is not None else []
        header += ["element face 8", "property list uchar uint vertex_indices", "end_header"]
        body = b"".join(struct.pack("<3f", *v[i]) + (bytes(colours[i]) if colours is not None else b"") for i in range(6))
        body += b"".join(struct.pack("<B3I", 3, *f[i]) for i in range(8))
        assert loaders.meshPLYBytes(plain) == ("\n".join(header) + "\n").encode("ascii") + body, "a mesh without normals writes the bytes it always did"
        assert loaders.meshPLYBytes(dict(plain, normals=None)) == loaders.meshPLYBytes(plain)
        path = tmp_path / "plain.ply"
        loaders.saveMeshPLY(str(path), plain)
        back = loaders.loadMeshPLY(str(path))
        assert set(back) == {"vertices", "faces", "colours"}
        path = tmp_path / "normals.ply"
        loaders.saveMeshPLY(str(path), dict(plain, normals=n))
        back = loaders.loadMeshPLY(str(path))
        assert back["normals"].dtype == np.float32 and back["normals"].tobytes() == n.tobytes()
        assert back["vertices"].tobytes() == v.tobytes() and back["faces"].tobytes() == f.tobytes()
        assert (back["colours"] is None) if colours is None else back["colours"].tobytes() == c.tobytes()
        assert b"property float nx\nproperty float ny\nproperty float nz\n" in path.read_bytes()
        assert len(path.read_bytes()) == len(loaders.meshPLYBytes(plain)) + 3 * len("property float nx\n") + 6 * 12
    with pytest.raises(ValueError):
        loaders.meshPLYBytes(dict(vertices=v, faces=f, colours=None, normals=n[:5]))
