"""Mesh connected components and small-component removal restated in plain numpy / Python (include/webdgs.h): a sequential
union-find that links the larger root under the smaller, numbering by ascending representative, the host selection rule and the compaction.  Every output
is an integer array; the GPU tests compare bytes.  Also the mesh shapes the CPU and the GPU tests share."""
import numpy as np

NONE = 0xFFFFFFFF


def components(faces, num_vertices):
    """``dict(count, faceComponent u32[F], vertexComponent u32[V], triangles u32[C], vertices u32[C], invalidFaces)`` of ``faces`` u32[F,3] over
    ``num_vertices`` vertices."""
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    V = int(num_vertices)
    valid = np.all(faces.astype(np.int64) < V, axis=1) if faces.size else np.zeros(0, bool)
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in faces[valid].tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)   # the lowest index of a set is its root
    root = np.array([find(v) for v in range(V)], np.int64).reshape(V)
    used = np.zeros(V, bool)
    used[root[faces[valid][:, 0].astype(np.int64)]] = True
    number = np.cumsum(used) - used   # exclusive scan: ascending representative
    C = int(used.sum())
    vcomp = np.where(used[root], number[root], NONE).astype(np.uint32) if V else np.zeros(0, np.uint32)
    fcomp = np.full(faces.shape[0], NONE, np.uint32)
    fcomp[valid] = number[root[faces[valid][:, 0].astype(np.int64)]]
    triangles = np.bincount(fcomp[valid].astype(np.int64), minlength=C).astype(np.uint32)
    vertices = np.bincount(vcomp[vcomp != NONE].astype(np.int64), minlength=C).astype(np.uint32)
    return dict(count=C, faceComponent=fcomp, vertexComponent=vcomp, triangles=triangles, vertices=vertices, invalidFaces=int((~valid).sum()))


def components_bfs(faces, num_vertices):
    """The same partition by an independent route: breadth-first search over a vertex adjacency built from the valid faces, vertices visited in ascending
    order (so components come out in ascending order of their lowest vertex).  Returns ``(vertexComponent, faceComponent)``."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(num_vertices)
    valid = np.all(faces < V, axis=1) if faces.size else np.zeros(0, bool)
    adjacency = [[] for _ in range(V)]
    named = np.zeros(V, bool)
    for a, b, c in faces[valid].tolist():
        adjacency[a] += [b, c]
        adjacency[b] += [a, c]
        adjacency[c] += [a, b]
        named[[a, b, c]] = True
    vcomp = np.full(V, NONE, np.uint32)
    count = 0
    for s in range(V):
        if not named[s] or vcomp[s] != NONE:
            continue
        vcomp[s] = count
        frontier = [s]
        while frontier:
            nxt = []
            for u in frontier:
                for w in adjacency[u]:
                    if vcomp[w] == NONE:
                        vcomp[w] = count
                        nxt.append(w)
            frontier = nxt
        count += 1
    fcomp = np.full(faces.shape[0], NONE, np.uint32)
    fcomp[valid] = vcomp[faces[valid][:, 0]]
    return vcomp, fcomp


def select(triangles, keepLargest=None, minTriangles=0, minFraction=0.0):
    """bool[C]: ranked by (triangles descending, component number ascending), kept when among the first ``keepLargest`` (None: all), with
    ``triangles >= minTriangles`` and ``triangles >= minFraction * largest`` in float64.  Written as a loop, unlike the product's."""
    t = [int(x) for x in np.asarray(triangles).reshape(-1)]
    ranking = sorted(range(len(t)), key=lambda c: (-t[c], c))
    keep = np.zeros(len(t), bool)
    for rank, c in enumerate(ranking):
        if keepLargest is not None and rank >= keepLargest:
            continue
        if t[c] >= minTriangles and float(t[c]) >= float(minFraction) * float(t[ranking[0]]):
            keep[c] = True
    return keep


def compact(mesh, labels, keep):
    """``dict(vertices, faces, vertexMap, faceMap, components)`` and ``colours`` / ``keys`` where ``mesh`` has them: kept faces in their order, kept vertices
    in ascending original index, faces rewritten."""
    faces = np.ascontiguousarray(mesh["faces"], np.uint32).reshape(-1, 3)
    vertices = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1, 3)
    keep = np.asarray(keep, bool)
    lookup = np.concatenate([keep, [False]])   # (the last entry serves 0xFFFFFFFF)
    index = lambda comp: np.where(comp == NONE, keep.size, comp).astype(np.int64)   # noqa: E731
    vkeep, fkeep = lookup[index(labels["vertexComponent"])], lookup[index(labels["faceComponent"])]
    vmap, fmap = np.flatnonzero(vkeep).astype(np.uint32), np.flatnonzero(fkeep).astype(np.uint32)
    new_index = np.cumsum(vkeep) - vkeep
    out = dict(vertices=vertices[vmap], faces=new_index[faces[fmap].astype(np.int64)].astype(np.uint32).reshape(-1, 3), vertexMap=vmap, faceMap=fmap,
               components=np.asarray(labels["triangles"], np.uint32)[keep])
    for name in ("colours", "keys"):
        if name in mesh:
            out[name] = None if mesh[name] is None else np.ascontiguousarray(np.asarray(mesh[name])[vmap])
    return out


def remove_small(mesh, keepLargest=None, minTriangles=0, minFraction=0.0):
    labels = components(mesh["faces"], np.asarray(mesh["vertices"]).reshape(-1, 3).shape[0])
    return compact(mesh, labels, select(labels["triangles"], keepLargest, minTriangles, minFraction))


# ---------------------------------------------------------------- the shapes (faces u32[F,3], V)
def _positions(V, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3)).astype(np.float32)


def as_mesh(faces, V, seed=5):
    return dict(vertices=_positions(V, seed), faces=np.ascontiguousarray(faces, np.uint32).reshape(-1, 3))


def clusters(V=5000, F=6000, seed=11):
    """About 300 components of mixed size (singletons included) over shuffled vertex numbers and face order, isolated vertices, degenerate faces, and
    invalid faces with an index = V and an index = 0xFFFFFFFF.  Components 0 .. are fans over consecutive vertex ranges before the shuffle."""
    rng = np.random.default_rng(seed)
    n_invalid, n_degenerate, n_single = 40, 60, 90
    sizes = [1] * n_single + [2] * 2 + [7] * 2 + [3, 5, 9, 12, 17]   # equal sizes on purpose: the selection's ties
    budget = F - n_invalid - n_degenerate
    while len(sizes) < 300:
        sizes.append(int(rng.integers(2, 40)))
    sizes = np.array(sizes)
    sizes[-1] += budget - sizes.sum()   # the last one takes what is left: the largest
    assert sizes[-1] > sizes[:-1].max() and sizes.sum() == budget
    faces, v0 = [], 0
    for s in sizes:   # a two-sided strip: s triangles over (s + 1) // 2 + 2 vertices
        m = (s + 1) // 2 + 2
        idx = v0 + np.arange(m - 2)
        front = np.stack([idx, idx + 1, idx + 2], axis=1)
        faces.append(np.concatenate([front, front[:, ::-1]])[:s])
        v0 += m
    faces = np.concatenate(faces)
    assert v0 + 50 <= V   # the rest: isolated vertices
    f = faces[rng.integers(0, faces.shape[0], n_degenerate)]
    degenerate = np.stack([f[:, 0], f[:, 0], np.where(np.arange(n_degenerate) % 2 == 0, f[:, 0], f[:, 2])], axis=1)   # (a, a, a) and (a, a, b), b of a's own strip
    invalid = faces[rng.integers(0, faces.shape[0], n_invalid)].astype(np.int64)
    invalid[::2, 1] = V
    invalid[1::2, 2] = NONE
    perm = rng.permutation(V)
    all_faces = np.concatenate([perm[faces], perm[degenerate], np.where(invalid >= V, invalid, perm[np.minimum(invalid, V - 1)])])
    all_faces = all_faces[rng.permutation(all_faces.shape[0])]
    assert all_faces.shape[0] == F
    return all_faces.astype(np.uint32), V


def chain(n=20000, numbering="ascending", seed=3):
    """A strip of n triangles; ``numbering``: ascending, descending (the deepest trees before flattening) or random."""
    idx = np.arange(n)
    faces = np.stack([idx, idx + 1, idx + 2], axis=1)
    V = n + 2
    if numbering == "descending":
        faces = V - 1 - faces
    elif numbering == "random":
        faces = np.random.default_rng(seed).permutation(V)[faces]
    return faces.astype(np.uint32), V


def star(n=50000, hub="lowest"):
    """n triangles that share one vertex and nothing else: every union contends on one root."""
    V = 2 * n + 1
    k = np.arange(n)
    if hub == "lowest":
        faces = np.stack([np.zeros(n, np.int64), 1 + 2 * k, 2 + 2 * k], axis=1)
    else:
        faces = np.stack([np.full(n, V - 1), 2 * k, 1 + 2 * k], axis=1)
    return faces.astype(np.uint32), V


def singletons(n=70000, seed=7):
    """n pairwise disjoint triangles over shuffled vertex numbers: C = F, more than one scan workgroup."""
    perm = np.random.default_rng(seed).permutation(3 * n)
    return perm.reshape(n, 3).astype(np.uint32), 3 * n


def late_bridge(n=10000, first=False):
    """Two strips of n triangles each, joined by one face only: the very last, or the very first."""
    a, _ = chain(n)
    b = a.astype(np.int64) + (n + 2)
    bridge = np.array([[n + 1, n + 2, 2 * n + 3]])
    parts = [bridge, a, b] if first else [a, b, bridge]
    return np.concatenate(parts).astype(np.uint32), 2 * n + 4


SHAPES = {
    "clusters": clusters,
    "chain-ascending": lambda: chain(numbering="ascending"),
    "chain-descending": lambda: chain(numbering="descending"),
    "chain-random": lambda: chain(numbering="random"),
    "star-low-hub": lambda: star(hub="lowest"),
    "star-high-hub": lambda: star(hub="highest"),
    "singletons": singletons,
    "bridge-last": lambda: late_bridge(first=False),
    "bridge-first": lambda: late_bridge(first=True),
    "no-faces": lambda: (np.zeros((0, 3), np.uint32), 17),
    "no-vertices": lambda: (np.array([[0, 1, 2], [NONE, 0, 0]], np.uint32), 0),
    "one-face": lambda: (np.array([[4, 2, 9]], np.uint32), 12),
    "only-invalid": lambda: (np.array([[0, 1, 5], [5, 5, 5], [NONE, 1, 2], [7, 0, 1]], np.uint32), 5),
}

_cache = {}


def shape(name):
    """``(faces, V, labels)`` of a named shape, computed once and shared (read-only)."""
    if name not in _cache:
        faces, V = SHAPES[name]()
        labels = components(faces, V)
        for a in [faces] + [x for x in labels.values() if isinstance(x, np.ndarray)]:
            a.setflags(write=False)
        _cache[name] = (faces, V, labels)
    return _cache[name]


# ---------------------------------------------------------------- two spheres in a TSDF volume
TS_DIMS = (40, 24, 24)
TS_VOXEL = 0.05
TS_TRUNC = 0.15
TS_ORIGIN = np.array([-1.0, -0.6, -0.6], np.float32)
TS_A = dict(centre=np.array([-0.4130, 0.0170, -0.0210]), radius=0.3350)   # off the lattice; the larger one
TS_B = dict(centre=np.array([0.5620, -0.0330, 0.0410]), radius=0.2050)


def two_sphere_fields():
    """``(T_both, T_a, W, rgb)`` float32 [nz, ny, nx] (rgb [3, nz, ny, nx]): min(d_A, d_B) / truncation clamped at 1, sphere A alone, unit weights and a
    smooth colour field."""
    nx, ny, nz = TS_DIMS
    o = TS_ORIGIN.astype(np.float64)
    z, y, x = np.meshgrid(o[2] + (np.arange(nz) + 0.5) * TS_VOXEL, o[1] + (np.arange(ny) + 0.5) * TS_VOXEL, o[0] + (np.arange(nx) + 0.5) * TS_VOXEL, indexing="ij")
    d = lambda s: np.sqrt((x - s["centre"][0]) ** 2 + (y - s["centre"][1]) ** 2 + (z - s["centre"][2]) ** 2) - s["radius"]   # noqa: E731
    da, db = d(TS_A), d(TS_B)
    both = np.minimum(np.minimum(da, db) / TS_TRUNC, 1.0).astype(np.float32)
    alone = np.minimum(da / TS_TRUNC, 1.0).astype(np.float32)
    rgb = np.stack([0.5 + 0.4 * np.sin(3 * x), 0.5 + 0.4 * np.cos(2 * y), 0.5 + 0.3 * np.sin(4 * z + x)]).astype(np.float32)
    return both, alone, np.ones(both.shape, np.float32), rgb
