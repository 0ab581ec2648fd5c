"""Mesh simplification by vertex clustering, restated in float32 and Python integers: ``sorted`` and loops, no ``np.unique``.
``simplify`` takes ``vertices f32[V,3]``, ``faces u32[F,3]``, ``colours u8[V,4] | None``, ``origin`` and ``cell_size`` and returns every output of
include/webdgs.h's definition; ``CASES`` are the crafted meshes the CPU and the GPU tests share."""
import functools

import numpy as np

U64_MAX = 2 ** 64 - 1
NONE = 0xFFFFFFFF
CELLS = 2 ** 21
F32 = np.float32


def cells_of(vertices, origin, cell_size):
    """``(t f32[V,3], c f32[V,3], inside bool[V])``: t = (p - origin) * inv and c = floor(t), every operation rounded once to float32."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    o = np.asarray(origin, F32).reshape(3)
    inv = F32(1.0) / F32(cell_size)
    with np.errstate(all="ignore"):
        d = v - o[None, :]
        t = d * inv
        c = np.floor(t)
        inside = np.all(np.isfinite(t), axis=1) & np.all(c >= 0, axis=1) & np.all(c < CELLS, axis=1)
    assert d.dtype == t.dtype == c.dtype == F32
    return t, c, inside


def simplify(vertices, faces, colours, origin, cell_size):
    """``dict(vertices f32[V',3], faces u32[F',3], colours u8[V',4] | None, keys u64[V'], faceMap u32[F'], vertexCluster u32[V], stats)``, ``stats`` the
    dict ``MeshSimplifier.stats`` returns: clusters, invalid, outside, collapsed, duplicate, vertices, faces."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    col = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 4)
    o = np.asarray(origin, F32).reshape(3)
    cell = F32(cell_size)
    assert np.all(np.isfinite(o)) and np.isfinite(cell) and cell > 0
    V, F = v.shape[0], f.shape[0]
    t, c, inside = cells_of(v, o, cell)
    keys, q = [], []
    for i in range(V):
        if not inside[i]:
            keys.append(U64_MAX)
            q.append(None)
            continue
        cx, cy, cz = (int(x) for x in c[i])
        keys.append((cz << 42) | (cy << 21) | cx)
        frac = t[i] - c[i]                                   # exact
        q.append([int(x) for x in (frac * F32(65536.0)).astype(np.uint32)])   # truncates
    # the clusters: the distinct inside keys in ascending order
    order = sorted(range(V), key=lambda i: (keys[i], i))
    cluster_of = [None] * V
    cluster_keys, members = [], []
    for n, i in enumerate(order):
        if keys[i] == U64_MAX:
            break
        if n == 0 or keys[i] != keys[order[n - 1]]:
            cluster_keys.append(keys[i])
            members.append([])
        cluster_of[i] = len(cluster_keys) - 1
        members[-1].append(i)
    C = len(cluster_keys)
    positions = np.zeros((C, 3), F32)
    ccol = np.zeros((C, 4), np.uint8)
    for k in range(C):
        n = len(members[k])
        for a in range(3):
            Q = sum(q[i][a] for i in members[k])
            qm = (2 * Q + n) // (2 * n)
            cc = (cluster_keys[k] >> (21 * a)) & (CELLS - 1)
            h = F32(qm) + F32(0.5)
            fr = h * F32(2.0 ** -16)
            s = F32(cc) + fr
            m = s * cell
            positions[k, a] = o[a] + m
            assert all(isinstance(x, np.float32) for x in (h, fr, s, m))
        if col is not None:
            for b in range(4):
                S = sum(int(col[i, b]) for i in members[k])
                ccol[k, b] = (2 * S + n) // (2 * n)
    # the faces
    counts = dict(invalid=0, outside=0, collapsed=0, duplicate=0)
    seen, kept = {}, []
    for j in range(F):
        idx = [int(x) for x in f[j]]
        if any(x >= V for x in idx):
            counts["invalid"] += 1
            continue
        if any(cluster_of[x] is None for x in idx):
            counts["outside"] += 1
            continue
        tri = [cluster_of[x] for x in idx]
        if tri[0] == tri[1] or tri[1] == tri[2] or tri[0] == tri[2]:
            counts["collapsed"] += 1
            continue
        lead = tri.index(min(tri))
        rotated = (tri[lead], tri[(lead + 1) % 3], tri[(lead + 2) % 3])
        if rotated in seen:
            counts["duplicate"] += 1
            continue
        seen[rotated] = j
        kept.append((j, tri))
    used = sorted({k for _, tri in kept for k in tri})
    new = {k: n for n, k in enumerate(used)}
    vertex_cluster = np.full(V, NONE, np.uint32)
    for i in range(V):
        if cluster_of[i] is not None and cluster_of[i] in new:
            vertex_cluster[i] = new[cluster_of[i]]
    stats = dict(clusters=C, vertices=len(used), faces=len(kept), **counts)
    return dict(vertices=np.ascontiguousarray(positions[used].reshape(-1, 3)), faces=np.array([[new[k] for k in tri] for _, tri in kept], np.uint32).reshape(-1, 3),
                colours=None if col is None else np.ascontiguousarray(ccol[used].reshape(-1, 4)), keys=np.array([cluster_keys[k] for k in used], np.uint64),
                faceMap=np.array([j for j, _ in kept], np.uint32), vertexCluster=vertex_cluster, stats=stats)


OUTPUTS = ("vertices", "faces", "colours", "keys", "faceMap", "vertexCluster")


# ---------------------------------------------------------------- the crafted meshes
def _colours(V, seed):
    """Colours of V vertices: random bytes, with 0 and 255 in every byte of the first two vertices when there are that many."""
    c = np.random.default_rng(2000 + seed).integers(0, 256, (V, 4), dtype=np.uint64).astype(np.uint8)
    if V >= 2:
        c[0], c[1] = 0, 255
    return c


def _mesh(vertices, faces, origin=(0.0, 0.0, 0.0), cell=1.0, seed=0, colours=True):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    return dict(vertices=v, faces=np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), colours=_colours(v.shape[0], seed) if colours else None,
                origin=np.asarray(origin, F32), cell=float(F32(cell)))


def _nothing():
    return _mesh(np.zeros((0, 3)), np.zeros((0, 3)))


def _no_vertices():
    return _mesh(np.zeros((0, 3)), [[0, 1, 2], [0, 0, 0], [NONE, 5, 0]])


def _no_faces():
    return _mesh([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.25, 0.5, 0.5], [-1.0, 0.0, 0.0], [7.5, 2.5, 1.5]], np.zeros((0, 3)), seed=1)


def _one_cell():
    return _mesh([[0.1, 0.2, 0.3], [0.9, 0.1, 0.5], [0.4, 0.8, 0.7]], [[0, 1, 2]], origin=(0, 0, 0), cell=1.0, seed=2)


def _three_cells():
    return _mesh([[0.1, 0.2, 0.3], [1.9, 0.1, 0.5], [0.4, 2.8, 0.7]], [[0, 1, 2]], origin=(-0.5, -0.25, 0.0), cell=0.75, seed=3)


def _on_cell_face():
    # p = origin + k * cell exactly (k = 3, 0, 5 on x; origin and cell are dyadic, so the products are exact): the vertex belongs to cell k, offset 0
    o, cell = np.array([0.5, -1.25, 2.0]), 0.25
    v = [[o[0] + 3 * cell, o[1] + 0.1, o[2] + 0.1], [o[0], o[1] + 2 * cell, o[2] + 0.3], [o[0] + 5 * cell, o[1] + 0.05, o[2] + 7 * cell], [o[0] + 0.3, o[1] + 0.6, o[2]]]
    return _mesh(v, [[0, 1, 2], [1, 2, 3], [0, 2, 3]], origin=o, cell=cell, seed=4)


def _ulp_below_origin():
    o = np.array([1.0, 2.0, -3.0], F32)
    below = np.nextafter(o, F32(-np.inf))
    v = [[below[0], 2.5, -2.5], [1.5, below[1], -2.5], [1.5, 2.5, below[2]], [o[0], o[1], o[2]], [2.5, 2.5, -2.5], [1.5, 3.5, -2.5], [1.5, 2.5, -1.5]]
    return _mesh(v, [[0, 4, 5], [1, 4, 5], [2, 4, 5], [3, 4, 5], [4, 5, 6], [3, 5, 6]], origin=o, cell=1.0, seed=5)


def _cell_limit():
    # c = 2^21 - 1 is the last cell, c = 2^21 is outside; on every axis
    top, out = CELLS - 0.5, float(CELLS)
    v = [[top, 0.5, 0.5], [0.5, top, 0.5], [0.5, 0.5, top], [out, 0.5, 0.5], [0.5, out, 0.5], [0.5, 0.5, out], [0.5, 0.5, 0.5], [top, top, top]]
    return _mesh(v, [[0, 1, 2], [6, 0, 1], [3, 0, 1], [4, 1, 2], [5, 2, 0], [7, 6, 0], [7, 1, 2]], seed=6)


def _non_finite():
    n, i = np.nan, np.inf
    v = [[n, 0.5, 0.5], [0.5, i, 0.5], [0.5, 0.5, -i], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [i, n, -i], [3e38, 0.5, 0.5], [2.5, 2.5, 2.5]]
    return _mesh(v, [[0, 3, 4], [1, 3, 4], [2, 3, 4], [3, 4, 5], [6, 4, 5], [7, 4, 5], [8, 4, 5]], seed=7)


def _bad_indices():
    v = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [-2.0, 0.5, 0.5]]
    # an invalid face that also names an outside vertex, or would collapse, is INVALID: the first class that applies
    return _mesh(v, [[0, 1, 2], [0, 1, 4], [NONE, 1, 2], [3, 3, NONE], [0, 0, 2 ** 31], [2, 1, 0], [3, 1, 2]], seed=8)


def _rotations():
    v = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]
    # (a, b, c), (b, c, a) and (a, c, b) over the same three cells: one duplicate, the reversed face kept
    return _mesh(v, [[0, 1, 2], [1, 2, 0], [0, 2, 1]], seed=9)


def _same_triple():
    # two distinct input triangles (no shared vertex) over the same three cells in the same cyclic order, the second one rotated: the lower index survives
    v = [[2.5, 0.5, 0.5], [0.5, 0.5, 0.5], [1.5, 3.5, 0.5], [0.1, 0.9, 0.2], [1.9, 3.1, 0.8], [2.2, 0.3, 0.6], [5.5, 5.5, 5.5]]
    return _mesh(v, [[6, 0, 1], [0, 1, 2], [3, 4, 5], [6, 1, 0]], seed=10)


def _hot_cell():
    # 30 000 vertices with distinct sub-cell offsets and colours in one cell, two vertices in two other cells, faces joining them
    n = 30000
    rng = np.random.default_rng(11)
    offs = (rng.permutation(65536)[:n].astype(np.float64) + 0.5) / 65536.0
    hot = np.stack([3.0 + offs, 1.0 + offs[::-1], 2.0 + (np.arange(n) % 4099) / 4099.0], axis=1)
    v = np.concatenate([hot, [[7.25, 1.5, 2.5], [3.5, 9.75, 2.5]]])
    faces = [[i, n, n + 1] for i in (0, 1, 4095, 4096, n - 1)] + [[n, n + 1, 17], [5, 6, n], [n + 1, n, 123]]
    return _mesh(v, faces, seed=11)


def _row(n):
    # n vertices in a row of cells of two vertices each (the last cell holds one when n is odd); faces over three consecutive cells, and one reversed
    def make():
        i = np.arange(n)
        v = np.stack([(i // 2) + 0.25 + 0.5 * (i % 2), 0.5 + 0.0 * i, 0.125 + (i % 7) / 8.0], axis=1)
        faces = [[j, j + 2, j + 4] for j in range(0, n - 4)] + [[4, 2, 0]]
        return _mesh(v, faces, seed=12 + n)
    return make


def _random(colours, V=20481, F=40000, seed=20, cells=16):
    def make():
        rng = np.random.default_rng(seed)
        v = rng.uniform(0.0, 1.0, (V, 3)).astype(F32)
        v[rng.integers(0, V, 40)] = np.array([np.nan, 0.5, 0.5], F32)
        v[rng.integers(0, V, 40), 1] = F32(-0.25)
        v[rng.integers(0, V, 40), 2] = F32(1.0)   # still inside: cell `cells` of the grid
        local = np.argsort(v[:, 0], kind="stable").astype(np.int64)   # neighbours along x: faces that often collapse
        a = rng.integers(0, V - 2, F // 4)
        f = np.concatenate([rng.integers(0, V, (F - F // 4 - 1000, 3)), np.stack([local[a], local[a + 1], local[a + 2]], axis=1)])
        dup = f[rng.integers(0, f.shape[0], 1000)]
        dup = np.where(rng.integers(0, 2, (1000, 1)) == 0, dup[:, [1, 2, 0]], dup[:, [0, 2, 1]])   # rotated: a duplicate; reversed: another face
        f = np.concatenate([f, dup])
        f = f[rng.permutation(f.shape[0])]
        f[rng.integers(0, F, 25), rng.integers(0, 3, 25)] = V + rng.integers(0, 5, 25)
        f[7, 2] = NONE
        return _mesh(v, f, cell=1.0 / cells, seed=seed, colours=colours)
    return make


CASES = {"nothing": _nothing, "no-vertices": _no_vertices, "no-faces": _no_faces, "one-cell": _one_cell, "three-cells": _three_cells, "on-cell-face": _on_cell_face,
         "ulp-below-origin": _ulp_below_origin, "cell-limit": _cell_limit, "non-finite": _non_finite, "bad-indices": _bad_indices, "rotations": _rotations,
         "same-triple": _same_triple, "hot-cell": _hot_cell, "row-63": _row(63), "row-64": _row(64), "row-65": _row(65), "row-4097": _row(4097),
         "random": _random(True), "random-no-colours": _random(False),
         # F = 100 000: several blocks of the face scans, and second keys (a * 2^32 | rank) whose five low bytes all vary
         "many-faces": _random(True, V=30000, F=100000, seed=21, cells=64)}
# what the definition gives, where the case is about it: (V', F') and the class counts
EXPECT = {"nothing": dict(vertices=0, faces=0, clusters=0), "no-vertices": dict(vertices=0, faces=0, invalid=3), "no-faces": dict(vertices=0, faces=0, clusters=3),
          "one-cell": dict(vertices=0, faces=0, collapsed=1, clusters=1), "three-cells": dict(vertices=3, faces=1, clusters=3),
          "ulp-below-origin": dict(outside=3, faces=3), "cell-limit": dict(outside=3, faces=4), "non-finite": dict(outside=5, faces=2),
          "bad-indices": dict(invalid=4, outside=1, faces=2, duplicate=0), "rotations": dict(duplicate=1, faces=2, vertices=3, collapsed=0),
          "same-triple": dict(duplicate=1, faces=3), "hot-cell": dict(clusters=3, vertices=3, faces=2, collapsed=1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """The mesh of that name: ``dict(vertices, faces, colours | None, origin, cell)``; computed once and shared: callers leave it unchanged."""
    m = CASES[name]()
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name):
    """``simplify`` of that case; computed once and shared: callers leave it unchanged."""
    m = case(name)
    out = simplify(m["vertices"], m["faces"], m["colours"], m["origin"], m["cell"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def digest(result):
    """sha256 over the result's arrays in a fixed order, then its counts (what bindings/napi/meshsimplify_run.js prints)."""
    import hashlib
    h = hashlib.sha256()
    for k in OUTPUTS:
        if result[k] is not None:
            h.update(np.ascontiguousarray(result[k]).tobytes())
    h.update(np.array([result["stats"][k] for k in ("clusters", "invalid", "outside", "collapsed", "duplicate", "vertices", "faces")], np.uint32).tobytes())
    return h.hexdigest()
