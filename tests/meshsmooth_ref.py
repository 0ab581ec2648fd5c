"""Mesh adjacency, Taubin smoothing and area-weighted vertex normals, restated in float32 scalars and Python integers: ``sorted`` and
loops, no ``np.unique`` and no sum whose order numpy chooses.  ``adjacency`` takes ``faces u32[F,3]`` and ``V``; ``smooth`` and ``normals`` take the positions
as well and return every output of include/webdgs.h's definition; ``CASES`` are the crafted meshes the CPU and the GPU tests share."""
import functools
import math

import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
STATS = ("directedEdges", "edges", "boundaryEdges", "nonManifoldEdges", "invalidFaces", "boundaryVertices", "isolatedVertices", "maxDegree")
ZERO = F32(0.0)


def half_edges(faces, V):
    """``(pairs, invalid)``: the ``(key, slot)`` pairs of the valid faces in ascending (key, slot) order -- the stable sort's order -- and the invalid faces'
    number.  The slots of an invalid face (key 2^64 - 1) are left out: they contribute nothing."""
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    pairs, invalid = [], 0
    for i in range(f.shape[0]):
        c = [int(x) for x in f[i]]
        if any(x >= V for x in c) or c[0] == c[1] or c[1] == c[2] or c[0] == c[2]:
            invalid += 1
            continue
        for j in range(3):
            a, b = c[j], c[(j + 1) % 3]
            pairs.append(((a << 32) | b, 6 * i + 2 * j))
            pairs.append(((b << 32) | a, 6 * i + 2 * j + 1))
    return sorted(pairs), invalid


def adjacency(faces, V):
    """``dict(rowStart u32[V+1], neighbours u32[E], boundary u32[V], stats, multiplicity: list, slots: list per vertex of its sorted slots)``."""
    pairs, invalid = half_edges(faces, V)
    rows = [[] for _ in range(V)]      # per vertex: [neighbour, multiplicity], ascending
    slots = [[] for _ in range(V)]     # per vertex: its slots in sorted order
    last = None
    for key, slot in pairs:
        a, b = key >> 32, key & NONE
        slots[a].append(slot)
        if key == last:
            rows[a][-1][1] += 1
        else:
            rows[a].append([b, 1])
            last = key
    row_start, neighbours, multiplicity = [0], [], []
    boundary = [0] * V
    boundary_edges = non_manifold = 0
    for v in range(V):
        for u, m in rows[v]:
            neighbours.append(u)
            multiplicity.append(m)
            if m == 1:
                boundary[v] = 1
                boundary[u] = 1
            if v < u:
                boundary_edges += m == 1
                non_manifold += m >= 3
        row_start.append(len(neighbours))
    E = len(neighbours)
    assert E % 2 == 0
    stats = dict(directedEdges=E, edges=E // 2, boundaryEdges=boundary_edges, nonManifoldEdges=non_manifold, invalidFaces=invalid, boundaryVertices=sum(boundary),
                 isolatedVertices=sum(1 for r in rows if not r), maxDegree=max([len(r) for r in rows] or [0]))
    return dict(rowStart=np.array(row_start, np.uint32), neighbours=np.array(neighbours, np.uint32), boundary=np.array(boundary, np.uint32), stats=stats,
                multiplicity=multiplicity, slots=slots)


def _finite(p):
    return bool(np.isfinite(p[0]) and np.isfinite(p[1]) and np.isfinite(p[2]))


def step(p, adj, w, pin_boundary):
    """One smoothing step over positions ``p`` f32[V,3]: a new array."""
    V = p.shape[0]
    w = F32(w)
    out = p.copy()
    rs, nb, bd = adj["rowStart"], adj["neighbours"], adj["boundary"]
    finite = [_finite(p[v]) for v in range(V)]
    with np.errstate(all="ignore"):
        for v in range(V):
            if (pin_boundary and bd[v] == 1) or not finite[v]:
                continue
            s = [ZERO, ZERO, ZERO]
            n = 0
            for e in range(int(rs[v]), int(rs[v + 1])):
                u = int(nb[e])
                if not finite[u]:
                    continue
                for a in range(3):
                    s[a] = s[a] + p[u, a]
                n += 1
            if n == 0:
                continue
            r = []
            for a in range(3):
                m = s[a] / F32(n)
                d = m - p[v, a]
                t = w * d
                r.append(p[v, a] + t)
                assert all(isinstance(x, np.float32) for x in (s[a], m, d, t, r[-1]))
            if _finite(r):
                out[v] = r
    return out


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, adj=None):
    """``vertices`` after ``iterations`` rounds of ``step(lam)`` then ``step(mu)``; a weight of exactly 0 skips its step."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3).copy()
    adj = adjacency(faces, p.shape[0]) if adj is None else adj
    for _ in range(iterations):
        for w in (lam, mu):
            if F32(w) != 0:
                p = step(p, adj, w, pin_boundary)
    return p


def normals(vertices, faces, adj=None):
    """The area-weighted vertex normals f32[V,3]: per vertex the forward slots of its run in sorted slot order, g_f from the face's own corner order."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    V = p.shape[0]
    adj = adjacency(f, V) if adj is None else adj
    out = np.zeros((V, 3), F32)
    cross = {}
    with np.errstate(all="ignore"):
        for v in range(V):
            s = [ZERO, ZERO, ZERO]
            n = 0
            for slot in adj["slots"][v]:
                if slot & 1:
                    continue
                i = slot // 6
                if i not in cross:
                    c0, c1, c2 = (int(x) for x in f[i])
                    a, b = p[c1] - p[c0], p[c2] - p[c0]
                    cross[i] = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
                g = cross[i]
                if not _finite(g):
                    continue
                for k in range(3):
                    s[k] = s[k] + g[k]
                n += 1
            q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
            assert isinstance(q, np.float32)
            if n == 0 or q == 0 or not np.isfinite(q):
                continue
            length = np.sqrt(q)
            out[v] = [s[0] / length, s[1] / length, s[2] / length]
    return out


# ---------------------------------------------------------------- the crafted meshes
def _mesh(vertices, faces, **smoothing):
    """``smoothing``: the arguments of the case's smoothing run (``iterations``, ``lam``, ``mu``, ``pin_boundary``); two default iterations otherwise."""
    return dict(vertices=np.ascontiguousarray(vertices, F32).reshape(-1, 3), faces=np.ascontiguousarray(faces, np.uint32).reshape(-1, 3),
                smoothing=dict(dict(iterations=2, lam=0.5, mu=-0.53, pin_boundary=True), **smoothing))


def _positions(V, seed):
    return np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, (V, 3)).astype(F32)


TETRAHEDRON = ([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
OCTAHEDRON = ([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]],
              [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def icosphere(subdivisions):
    """``(vertices f64[V,3], faces)`` of the unit icosphere, outward wound: 12, 42, 162, ... vertices."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    v = [list(np.array(x) / np.linalg.norm(x)) for x in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6],
         [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(subdivisions):
        mid, g = {}, []

        def middle(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = (np.array(v[a]) + np.array(v[b])) / 2.0
                v.append(list(m / np.linalg.norm(m)))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = g
    return np.array(v, np.float64), f


def noisy_icosphere(seed=7, sigma=0.03):
    """The 162-vertex unit icosphere with radii 1 + N(0, sigma): ``(vertices f64, faces)``."""
    v, f = icosphere(2)
    r = 1.0 + sigma * np.random.default_rng(seed).standard_normal(v.shape[0])
    return v * r[:, None], f


def _fan(n, **smoothing):
    """A hub (vertex 0) with n rim vertices and n - 1 faces: the hub's row has n neighbours."""
    def make():
        ang = np.arange(n) * (1.5 * math.pi / n)
        v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(7 * ang)], axis=1)])
        return _mesh(v, [[0, i, i + 1] for i in range(1, n)], pin_boundary=False, iterations=1, **smoothing)
    return make


def _random(V, F, seed, **smoothing):
    def make():
        rng = np.random.default_rng(seed)
        f = rng.integers(0, V, (F, 3))
        f[rng.integers(0, F, 5), rng.integers(0, 3, 5)] = V + rng.integers(0, 3, 5)
        return _mesh(_positions(V, seed), f, pin_boundary=False, **smoothing)
    return make


def _tail_used():
    V, used = 10000, 50
    base = V - used
    faces = [[base + i, base + i + 1, base + i + 2] for i in range(used - 2)]
    return _mesh(_positions(V, 1), faces, pin_boundary=False)


def _first_unused():
    return _mesh(_positions(6, 2), [[1, 2, 5], [2, 3, 5], [5, 3, 1]], pin_boundary=False)


def _non_finite():
    n, i = np.nan, np.inf
    # a ring of eight around vertex 0; vertex 3 is NaN, vertex 5 +inf: both are neighbours of finite vertices and vertices with finite neighbours
    ang = np.arange(8) * (2 * math.pi / 8)
    v = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], axis=1)])
    v[3] = [n, 0.5, 0.5]
    v[5] = [0.25, i, -0.5]
    return _mesh(v, [[0, k, k % 8 + 1] for k in range(1, 9)], pin_boundary=False, iterations=3)


def _overflow():
    # rim vertices 1 and 2 together pass the largest float on x: the sums of the hub and of rim vertices 3 and 4 are +inf and those three are copied;
    # vertices 1 and 2 have small sums and move (one step: they come down to 1.5e38, and the next step's sums are finite)
    big = 3.0e38
    v = [[0.0, 0.0, 0.0], [big, 1.0, 0.0], [big, -1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]]
    return _mesh(v, [[0, 1, 3], [0, 3, 2], [0, 2, 4], [0, 4, 1]], pin_boundary=False, iterations=1, mu=0.0)


def _noisy():
    v, f = noisy_icosphere()
    return _mesh(v, f, iterations=3)


def _grid(n, **smoothing):
    """An open n x n grid of quads split in two, with a ripple: an interior that moves and a boundary to pin."""
    def make():
        ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
        v = np.stack([ij[:, 0] / (n - 1.0), ij[:, 1] / (n - 1.0), 0.05 * np.sin(3.0 * ij[:, 0]) * np.cos(2.0 * ij[:, 1])], axis=1)
        f = []
        for i in range(n - 1):
            for j in range(n - 1):
                a = i * n + j
                f += [[a, a + n, a + 1], [a + 1, a + n, a + n + 1]]
        return _mesh(v, f, **smoothing)
    return make


CASES = {
    "nothing": lambda: _mesh(np.zeros((0, 3)), np.zeros((0, 3))),
    "no-vertices": lambda: _mesh(np.zeros((0, 3)), [[0, 1, 2], [NONE, 5, 0]]),
    "no-faces": lambda: _mesh(_positions(5, 0), np.zeros((0, 3))),
    "triangle-pinned": lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2]]),
    "triangle-unpinned": lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2]], pin_boundary=False),
    "two-triangles": lambda: _mesh([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [1, 1, -0.3]], [[0, 1, 2], [2, 1, 3]], pin_boundary=False),
    "tetrahedron": lambda: _mesh(*TETRAHEDRON),
    "octahedron": lambda: _mesh(*OCTAHEDRON),
    "fin": lambda: _mesh([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 0.8, 0.5], [-0.5, -0.8, 0.4]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]], pin_boundary=False),
    "same-face-twice": lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0.5], [1, 1, 1]], [[0, 1, 2], [1, 2, 0], [2, 1, 3]], pin_boundary=False),
    "both-orientations": lambda: _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2], [0, 2, 1]], pin_boundary=False),
    "bad-indices": lambda: _mesh(_positions(5, 3), [[0, 1, 2], [0, 1, 5], [NONE, 1, 2], [3, 3, 4], [2, 1, 3], [4, 4, 4], [2 ** 31, 0, 1]], pin_boundary=False),
    "non-finite": _non_finite,
    "overflow": _overflow,
    "fan-63": _fan(63), "fan-64": _fan(64), "fan-65": _fan(65), "fan-5000": _fan(5000),
    "tail-used": _tail_used,
    "first-unused": _first_unused,
    # 6 F = 4092 and 4098: either side of the sort's tile of 4096 slots (keysort_tiling)
    "tile-below": _random(300, 682, 30, iterations=1), "tile-above": _random(300, 683, 31, iterations=1),
    "many-faces": _random(30000, 100000, 32, iterations=1),      # several scan blocks
    "random": _random(20481, 40000, 33, iterations=1),           # non-manifold throughout
    "grid-pinned": _grid(9), "grid-laplacian": _grid(9, mu=0.0, iterations=3), "grid-mu-only": _grid(9, lam=0.0, iterations=3),
    "noisy-icosphere": _noisy,
}
# what the definition gives, where the case is about it
EXPECT = {"nothing": dict(directedEdges=0, invalidFaces=0, isolatedVertices=0, maxDegree=0), "no-vertices": dict(directedEdges=0, invalidFaces=2),
          "no-faces": dict(directedEdges=0, isolatedVertices=5), "triangle-pinned": dict(edges=3, boundaryEdges=3, boundaryVertices=3),
          "two-triangles": dict(edges=5, boundaryEdges=4, nonManifoldEdges=0, maxDegree=3), "tetrahedron": dict(edges=6, boundaryEdges=0, nonManifoldEdges=0),
          "octahedron": dict(edges=12, boundaryEdges=0, nonManifoldEdges=0), "fin": dict(edges=7, boundaryEdges=6, nonManifoldEdges=1),
          "same-face-twice": dict(edges=5, boundaryEdges=2, nonManifoldEdges=1), "both-orientations": dict(edges=3, boundaryEdges=0, nonManifoldEdges=0),
          "bad-indices": dict(invalidFaces=5, edges=5), "fan-5000": dict(maxDegree=5000, boundaryEdges=5001), "tail-used": dict(isolatedVertices=9950),
          "first-unused": dict(isolatedVertices=2, maxDegree=3)}


@functools.lru_cache(maxsize=None)
def case(name):
    """The mesh of that name: ``dict(vertices, faces, smoothing)``; computed once and shared: callers leave it unchanged."""
    m = CASES[name]()
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name):
    """``dict(rowStart, neighbours, boundary, stats, smoothed, normals)`` of that case -- ``smoothed`` by the case's own smoothing arguments, ``normals`` of
    the case's unsmoothed positions; computed once and shared: callers leave it unchanged."""
    m = case(name)
    adj = adjacency(m["faces"], m["vertices"].shape[0])
    out = dict(rowStart=adj["rowStart"], neighbours=adj["neighbours"], boundary=adj["boundary"], stats=adj["stats"],
               smoothed=smooth(m["vertices"], m["faces"], adj=adj, **m["smoothing"]), normals=normals(m["vertices"], m["faces"], adj=adj))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


OUTPUTS = ("rowStart", "neighbours", "boundary", "smoothed", "normals")


def digest(result):
    """sha256 over the result's arrays in a fixed order, then its statistics (what a host's run script prints)."""
    import hashlib
    h = hashlib.sha256()
    for k in OUTPUTS:
        h.update(np.ascontiguousarray(result[k]).tobytes())
    h.update(np.array([result["stats"][k] for k in STATS], np.uint32).tobytes())
    return h.hexdigest()
