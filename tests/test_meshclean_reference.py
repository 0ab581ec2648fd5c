"""CPU: the restatement of mesh connected components and small-component removal (tests/meshclean_ref.py) against an independent breadth-first search on
every shape the GPU tests use, its invariances under a permutation of the faces, the selection's tie rule, idempotence of the compaction, and the
two-sphere property of the TSDF mesh restatement (tests/tsdf64.py) that tests/test_gpu_meshclean.py relies on."""
import numpy as np
import pytest

import meshclean_ref as M
import tsdf64 as t64


@pytest.mark.parametrize("name", sorted(M.SHAPES))
def test_restatement_equals_breadth_first_search(name):
    faces, V, got = M.shape(name)
    vcomp, fcomp = M.components_bfs(faces, V)
    assert np.array_equal(got["vertexComponent"], vcomp) and np.array_equal(got["faceComponent"], fcomp)
    C = got["count"]
    assert C == (int(vcomp[vcomp != M.NONE].max()) + 1 if np.any(vcomp != M.NONE) else 0)
    assert np.array_equal(got["triangles"], np.bincount(fcomp[fcomp != M.NONE], minlength=C))
    assert np.array_equal(got["vertices"], np.bincount(vcomp[vcomp != M.NONE], minlength=C))
    assert got["invalidFaces"] == int(np.sum(fcomp == M.NONE)) and int(got["triangles"].sum()) + got["invalidFaces"] == faces.shape[0]
    assert np.all(got["triangles"] >= 1)
    # numbered in ascending order of the lowest vertex
    lowest = np.full(C, V, np.int64)
    np.minimum.at(lowest, vcomp[vcomp != M.NONE].astype(np.int64), np.flatnonzero(vcomp != M.NONE))
    assert np.all(np.diff(lowest) > 0)


def test_shapes_are_what_the_issue_describes():
    faces, V, lab = M.shape("clusters")
    assert (V, faces.shape[0]) == (5000, 6000) and 250 <= lab["count"] <= 350 and lab["invalidFaces"] == 40
    assert np.sum(lab["triangles"] == 1) >= 20 and np.sum(lab["vertexComponent"] == M.NONE) >= 50
    assert np.any(faces == V) and np.any(faces == M.NONE) and np.any((faces[:, 0] == faces[:, 1]) & (faces[:, 1] == faces[:, 2]))
    for name in ("chain-ascending", "chain-descending", "chain-random"):
        _, _, lab = M.shape(name)
        assert lab["count"] == 1 and lab["triangles"].tolist() == [20000]
    for name in ("star-low-hub", "star-high-hub"):
        _, _, lab = M.shape(name)
        assert lab["count"] == 1 and lab["triangles"].tolist() == [50000] and lab["vertices"].tolist() == [100001]
    faces, V, lab = M.shape("singletons")
    assert lab["count"] == faces.shape[0] == 70000 and np.array_equal(np.argsort(faces.min(axis=1), kind="stable").argsort(), lab["faceComponent"])
    for name in ("bridge-last", "bridge-first"):
        _, _, lab = M.shape(name)
        assert lab["count"] == 1 and lab["triangles"].tolist() == [20001]
    assert M.shape("no-faces")[2]["count"] == 0 and M.shape("only-invalid")[2]["count"] == 0 and M.shape("only-invalid")[2]["invalidFaces"] == 4
    assert M.shape("no-vertices")[2]["invalidFaces"] == 2 and M.shape("one-face")[2]["vertices"].tolist() == [3]


@pytest.mark.parametrize("name", ["clusters", "chain-random", "bridge-last"])
def test_partition_and_numbering_do_not_depend_on_the_order_of_the_faces(name):
    faces, V, lab = M.shape(name)
    order = np.random.default_rng(19).permutation(faces.shape[0])
    got = M.components(faces[order], V)
    assert np.array_equal(got["vertexComponent"], lab["vertexComponent"])        # the numbering, hence the partition
    assert np.array_equal(got["faceComponent"], lab["faceComponent"][order])
    assert np.array_equal(got["triangles"], lab["triangles"]) and np.array_equal(got["vertices"], lab["vertices"])
    rolled = np.roll(faces, 1, axis=1)                                              # ... nor on which corner comes first
    assert np.array_equal(M.components(rolled, V)["faceComponent"], lab["faceComponent"])


def test_selection_rule_and_its_ties():
    t = np.array([5, 9, 5, 1, 9, 2], np.uint32)
    assert M.select(t).all()
    assert M.select(t, keepLargest=1).tolist() == [False, True, False, False, False, False]       # 9 twice: the lower number
    assert M.select(t, keepLargest=2).tolist() == [False, True, False, False, True, False]
    assert M.select(t, keepLargest=3).tolist() == [True, True, False, False, True, False]         # 5 twice: the lower number
    assert M.select(t, keepLargest=0).tolist() == [False] * 6 and M.select(t, keepLargest=99).all()
    assert M.select(t, minTriangles=5).tolist() == [True, True, True, False, True, False]         # a value two components share: both stay
    assert M.select(t, minFraction=5 / 9).tolist() == [True, True, True, False, True, False]
    assert M.select(t, minFraction=0.56).tolist() == [False, True, False, False, True, False]
    assert M.select(t, keepLargest=3, minTriangles=6).tolist() == [False, True, False, False, True, False]
    assert M.select(np.zeros(0, np.uint32), keepLargest=1).size == 0
    big = np.array([2 ** 31 - 1, 2 ** 31 - 2], np.uint32)
    assert M.select(big, minFraction=1.0).tolist() == [True, False]                                 # compared in float64, not float32


def test_product_selection_equals_the_restatement():
    from webdgs_amd import ops
    rng = np.random.default_rng(2)
    for _ in range(200):
        t = rng.integers(1, 8, int(rng.integers(0, 12))).astype(np.uint32)
        k = None if rng.random() < 0.3 else int(rng.integers(0, 14))
        m, f = int(rng.integers(0, 9)), float(rng.choice([0.0, 0.25, 0.5, 1 / 3, 1.0]))
        assert np.array_equal(ops.selectComponents(t, k, m, f), M.select(t, k, m, f)), (t, k, m, f)


def test_compaction_keeps_order_and_is_idempotent():
    faces, V, lab = M.shape("clusters")
    mesh = M.as_mesh(faces, V)
    mesh["keys"] = np.arange(V, dtype=np.uint64) * np.uint64(3)
    mesh["colours"] = (np.arange(3 * V) % 251).astype(np.uint8).reshape(V, 3)
    for kw in (dict(), dict(keepLargest=2), dict(minTriangles=7), dict(keepLargest=0)):
        out = M.remove_small(mesh, **kw)
        keep = M.select(lab["triangles"], **kw)
        assert np.all(np.diff(out["faceMap"].astype(np.int64)) > 0) and np.all(np.diff(out["vertexMap"].astype(np.int64)) > 0)
        assert out["faces"].shape[0] == int(lab["triangles"][keep].sum()) and out["vertices"].shape[0] == int(lab["vertices"][keep].sum())
        assert np.array_equal(out["vertexMap"][out["faces"]], faces[out["faceMap"]])             # the same triangles over the old indices
        assert np.array_equal(out["vertices"], mesh["vertices"][out["vertexMap"]]) and np.array_equal(out["keys"], mesh["keys"][out["vertexMap"]])
        again = M.remove_small(out, **kw)
        for k in ("vertices", "faces", "colours", "keys", "components"):
            assert np.array_equal(again[k], out[k]), (kw, k)
        assert np.array_equal(again["vertexMap"], np.arange(out["vertices"].shape[0])) and np.array_equal(again["faceMap"], np.arange(out["faces"].shape[0]))
    everything = M.remove_small(mesh)
    valid = lab["faceComponent"] != M.NONE
    assert np.array_equal(everything["faceMap"], np.flatnonzero(valid)) and everything["vertices"].shape[0] == int(np.sum(lab["vertexComponent"] != M.NONE))


def _weld(tri):
    vertices, faces = t64.weld(tri["keys"], tri["positions"])
    return dict(vertices=vertices.astype(np.float32), faces=faces.astype(np.uint32), keys=np.unique(tri["keys"].reshape(-1)))


def test_two_spheres_are_two_closed_components_and_the_larger_is_the_mesh_of_sphere_a_alone():
    both, alone, W, _ = M.two_sphere_fields()
    gap = np.linalg.norm(M.TS_A["centre"] - M.TS_B["centre"]) - M.TS_A["radius"] - M.TS_B["radius"]
    assert gap > M.TS_TRUNC + np.sqrt(3) * M.TS_VOXEL and M.TS_A["radius"] != M.TS_B["radius"]
    assert not np.any(np.abs((M.TS_A["centre"] - M.TS_ORIGIN) / M.TS_VOXEL - 0.5) % 1 < 0.05)     # off the lattice
    two = _weld(t64.mesh64(both, W, M.TS_ORIGIN, M.TS_VOXEL))
    one = _weld(t64.mesh64(alone, W, M.TS_ORIGIN, M.TS_VOXEL))
    lab = M.components(two["faces"], two["vertices"].shape[0])
    assert lab["count"] == 2 and lab["invalidFaces"] == 0
    for c in range(2):
        topo = t64.mesh_topology(two["faces"][lab["faceComponent"] == c])
        assert topo["closed"] and topo["consistent"] and topo["V"] - topo["E"] + topo["F"] == 2, (c, topo)
    kept = M.remove_small(two, keepLargest=1)
    assert kept["faces"].shape[0] == int(lab["triangles"].max()) > int(lab["triangles"].min())
    for k in ("vertices", "faces", "keys"):
        assert kept[k].tobytes() == one[k].tobytes(), k
