"""No GPU: the properties of vertex-clustering simplification as include/webdgs.h defines it, checked on the numpy restatement
(tests/meshsimplify_ref.py) over every crafted mesh the GPU test compares the device with."""
import numpy as np
import pytest

import meshsimplify_ref as S

NAMES = sorted(S.CASES)
# meshes whose coordinates, origin and cell size are dyadic with few bits, every vertex inside: a translation by whole cells is exact in float32
DYADIC = ("rotations", "row-63", "row-64", "row-65")


def _run(m, **changes):
    m = dict(m, **changes)
    return S.simplify(m["vertices"], m["faces"], m["colours"], m["origin"], m["cell"])


def _rotated(faces):
    """Every face rotated so that its smallest index comes first, as tuples."""
    out = []
    for a, b, c in np.asarray(faces).tolist():
        k = (a, b, c).index(min(a, b, c))
        out.append(((a, b, c), (b, c, a), (c, a, b))[k])
    return out


def _same(a, b, keys, what):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, f"{what}: {k}"
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"


@pytest.mark.parametrize("name", NAMES)
def test_outputs_are_a_clean_mesh_consistent_with_their_maps(name):
    m, r = S.case(name), S.expected(name)
    V, F = m["vertices"].shape[0], m["faces"].shape[0]
    nv, nf = r["vertices"].shape[0], r["faces"].shape[0]
    st = r["stats"]
    assert (st["vertices"], st["faces"]) == (nv, nf) and r["keys"].shape == (nv,) and r["faceMap"].shape == (nf,) and r["vertexCluster"].shape == (V,)
    assert r["vertices"].dtype == np.float32 and r["faces"].dtype == np.uint32 and r["keys"].dtype == np.uint64
    assert (r["colours"] is None) == (m["colours"] is None) and (r["colours"] is None or r["colours"].shape == (nv, 4))
    for k, want in S.EXPECT.get(name, {}).items():
        assert st[k] == want, f"{name}: {k} = {st[k]}, the case is built for {want}"
    # the five counts: every face is kept or dropped in exactly one class
    assert st["invalid"] + st["outside"] + st["collapsed"] + st["duplicate"] + nf == F
    assert st["clusters"] >= nv
    f = r["faces"].astype(np.int64)
    assert np.all(f < nv)
    assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])), "a face with a repeated index"
    rot = _rotated(f)
    assert len(set(rot)) == len(rot), "two faces equal up to rotation"
    assert np.array_equal(np.unique(f), np.arange(nv)), "a vertex that no face names"
    assert np.all(r["keys"][1:] > r["keys"][:-1]), "keys ascending and distinct"
    assert np.all(r["faceMap"][1:].astype(np.int64) > r["faceMap"][:-1].astype(np.int64)), "kept faces stay in input order"
    # the maps: every new face is its old face seen through vertex_cluster, corner by corner; every clustered vertex lies in its vertex's cell
    vc = r["vertexCluster"]
    assert np.all((vc == S.NONE) | (vc < nv))
    old = m["faces"][r["faceMap"]].astype(np.int64)
    assert np.array_equal(vc[old].reshape(-1, 3), r["faces"]) if nf else True
    t, c, inside = S.cells_of(m["vertices"], m["origin"], m["cell"])
    assert not np.any(vc[~inside] != S.NONE), "an outside vertex with a cluster"
    has = np.flatnonzero(vc != S.NONE)
    ci = c[has].astype(np.uint64)
    assert np.array_equal(r["keys"][vc[has]], (ci[:, 2] << np.uint64(42)) | (ci[:, 1] << np.uint64(21)) | ci[:, 0])


@pytest.mark.parametrize("name", NAMES)
def test_representatives_lie_in_their_cells(name):
    """The position is origin + (c + u) * cell with 0 < u < 1 before the last two operations, a multiply and an add, each rounded once: it lies in the box
    [origin + c cell, origin + (c + 1) cell] up to half an ulp of the product plus half an ulp of the sum -- one ulp of the largest magnitude involved."""
    m, r = S.case(name), S.expected(name)
    o, cell = m["origin"].astype(np.float64), float(m["cell"])
    for a in range(3):
        c = ((r["keys"] >> np.uint64(21 * a)) & np.uint64(S.CELLS - 1)).astype(np.float64)
        lo, hi = o[a] + c * cell, o[a] + (c + 1.0) * cell
        big = np.maximum(np.maximum(np.abs(lo), np.abs(hi)), (c + 1.0) * cell).astype(np.float32)
        slack = np.spacing(big).astype(np.float64)
        p = r["vertices"][:, a].astype(np.float64)
        assert np.all(p >= lo - slack) and np.all(p <= hi + slack), f"{name}: axis {a}"


def test_the_hot_cell_representative_is_the_rounded_integer_mean():
    m, r = S.case("hot-cell"), S.expected("hot-cell")
    n = 30000
    hot = int(r["vertexCluster"][0])
    assert np.all(r["vertexCluster"][:n] == hot)
    t, c, _ = S.cells_of(m["vertices"][:n], m["origin"], m["cell"])
    q = ((t - c) * np.float32(65536.0)).astype(np.uint32).astype(np.int64)
    assert np.unique(q[:, 0]).size == n, "the case has distinct sub-cell offsets"
    qm = (2 * q.sum(axis=0) + n) // (2 * n)
    want = (c[0].astype(np.float64) + (qm + 0.5) / 65536.0) * m["cell"] + m["origin"]
    assert np.allclose(r["vertices"][hot], want, rtol=0, atol=2e-6)
    col = m["colours"][:n].astype(np.int64)
    assert np.array_equal(r["colours"][hot], (2 * col.sum(axis=0) + n) // (2 * n))


@pytest.mark.parametrize("name", NAMES)
def test_permuting_the_faces_changes_neither_the_vertices_nor_the_set_of_faces(name):
    m, r = S.case(name), S.expected(name)
    F = m["faces"].shape[0]
    perm = np.random.default_rng(5).permutation(F)
    p = _run(m, faces=m["faces"][perm])
    _same(p, r, ("vertices", "colours", "keys", "vertexCluster"), name)
    assert set(_rotated(p["faces"])) == set(_rotated(r["faces"]))
    assert {k: v for k, v in p["stats"].items()} == r["stats"]


@pytest.mark.parametrize("name", NAMES)
def test_relabelling_the_vertices_changes_no_vertex_array(name):
    m, r = S.case(name), S.expected(name)
    V = m["vertices"].shape[0]
    perm = np.random.default_rng(6).permutation(V)          # new vertex i is old vertex perm[i]
    inverse = np.empty(V, np.int64)
    inverse[perm] = np.arange(V)
    f = m["faces"].astype(np.int64)
    valid = f < V
    relabelled = np.where(valid, inverse[np.where(valid, f, 0)] if V else f, f).astype(np.uint32)
    p = _run(m, vertices=m["vertices"][perm], colours=None if m["colours"] is None else m["colours"][perm], faces=relabelled)
    _same(p, r, ("vertices", "colours", "keys", "faces", "faceMap"), name)
    assert np.array_equal(p["vertexCluster"], r["vertexCluster"][perm]) and p["stats"] == r["stats"]


@pytest.mark.parametrize("name", DYADIC)
def test_a_translation_by_whole_cells_shifts_the_keys_and_nothing_else(name):
    m, r = S.case(name), S.expected(name)
    k = np.array([3, 1, 2])
    s = (k * m["cell"]).astype(np.float32)
    moved = m["vertices"] + s
    assert np.array_equal(moved.astype(np.float64), m["vertices"].astype(np.float64) + s.astype(np.float64)), "the case's translation is exact in float32"
    rest = ("faces", "colours", "faceMap", "vertexCluster")
    # the mesh and the origin moved together: the cells are the same, the representatives move along
    both = _run(m, vertices=moved, origin=m["origin"] + s)
    _same(both, r, rest + ("keys",), name)
    assert np.array_equal(both["vertices"], r["vertices"] + s) and both["stats"] == r["stats"]
    # the origin moved back alone: every cell index grows by k, and nothing else changes
    shifted = _run(m, origin=m["origin"] - s)
    _same(shifted, r, rest + ("vertices",), name)
    shift = (int(k[2]) << 42) | (int(k[1]) << 21) | int(k[0])
    assert np.array_equal(shifted["keys"], r["keys"] + np.uint64(shift)) and shifted["stats"] == r["stats"]


def test_bad_parameters_are_refused_by_the_restatement_too():
    m = S.case("three-cells")
    for cell in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(AssertionError):
            _run(m, cell=cell)
    with pytest.raises(AssertionError):
        _run(m, origin=np.array([0.0, np.nan, 0.0], np.float32))
