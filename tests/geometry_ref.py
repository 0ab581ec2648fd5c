"""The mesh accuracy metrics of csrc/geometry.hip restated in numpy float32, operation for operation: the GPU tests compare bytes.

``sample_mesh``, ``nearest`` (brute force over all pairs, with the tie rule) and ``distance_stats`` are the restatement; every array they compute on is float32
or an integer type, so each numpy operation is the one IEEE operation the kernel performs.  ``nearest64`` and ``barycentric64`` are float64 and serve only to
check the restatement (tests/test_geometry_reference.py)."""
import numpy as np

F32 = np.float32
U32 = np.uint32
NO_INDEX = 0xFFFFFFFF


# ---------------------------------------------------------------- the hash
def mix(x):
    x = np.asarray(x, U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7feb352d)
    x ^= x >> U32(15)
    x *= U32(0x846ca68b)
    x ^= x >> U32(16)
    return x


def sample_hash(seed, t, k, j):
    """h(seed, t, k, j), all u32 and wrapping; the arguments broadcast."""
    seed, t, k, j = (np.atleast_1d(np.asarray(a, np.uint64).astype(U32)) for a in (seed, t, k, j))
    return mix(mix(mix(mix(seed + U32(0x9E3779B9)) ^ t) + k) ^ (j * U32(0x85EBCA6B) + U32(1)))


def unit(h):
    return ((np.asarray(h, U32) >> U32(9)).astype(F32) + F32(0.5)) * F32(2.0 ** -23)


# ---------------------------------------------------------------- 1. sampling
def _corners(vertices, faces):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, U32).reshape(-1, 3)
    valid = np.all(f < v.shape[0], axis=1) if f.size else np.zeros(0, bool)
    safe = np.where(valid[:, None], f, 0).astype(np.int64) if v.shape[0] else np.zeros(f.shape, np.int64)
    if v.shape[0] == 0:
        z = np.zeros((f.shape[0], 3), F32)
        return z, z, z, valid
    return v[safe[:, 0]], v[safe[:, 1]], v[safe[:, 2]], valid


def sample_counts(vertices, faces, density, seed):
    """n_t per triangle (uint32)."""
    A, B, C, valid = _corners(vertices, faces)
    F = A.shape[0]
    density = F32(density)
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = F32(0.5) * np.sqrt((nx * nx + ny * ny) + nz * nz)
        x = area * density + unit(sample_hash(seed, np.arange(F), 0xFFFFFFFF, 0))
        assert x.dtype == F32
        fl = np.floor(x)
        n = np.where(np.isfinite(x) & valid & (fl > 0), np.minimum(fl, F32(2147483648.0)), F32(0)).astype(np.int64)
    return np.minimum(n, 2 ** 31 - 1).astype(U32)


def sample_mesh(vertices, faces, density, seed=0):
    """dict(points f32[total,3], face u32[total], counts u32[F], total int): sample k of triangle t at offsets[t] + k."""
    counts = sample_counts(vertices, faces, density, seed)
    total = int(counts.astype(np.int64).sum())
    if total >= 2 ** 31:
        raise OverflowError(f"{total} samples")
    A, B, C, _ = _corners(vertices, faces)
    t = np.repeat(np.arange(counts.size, dtype=np.int64), counts.astype(np.int64))
    offsets = np.cumsum(counts.astype(np.int64)) - counts
    k = np.arange(total, dtype=np.int64) - offsets[t]
    u, v = unit(sample_hash(seed, t, k, 1)), unit(sample_hash(seed, t, k, 2))
    flip = (u + v) > F32(1.0)
    u = np.where(flip, F32(1.0) - u, u)
    v = np.where(flip, F32(1.0) - v, v)
    A, B, C = A[t], B[t], C[t]
    e1, e2 = B - A, C - A
    points = (A + u[:, None] * e1) + v[:, None] * e2
    assert points.dtype == F32
    return dict(points=np.ascontiguousarray(points.reshape(total, 3)), face=t.astype(U32), counts=counts, total=total, u=u, v=v)


def barycentric64(points, vertices, faces, face):
    """float64 barycentrics (u, v) of each float32 point in the plane of its triangle, and its distance from that plane."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face, np.int64)]
    A, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    d = np.asarray(points, np.float64) - A
    a11, a12, a22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (d * e1).sum(1), (d * e2).sum(1)
    det = a11 * a22 - a12 * a12
    u, w = (b1 * a22 - b2 * a12) / det, (b2 * a11 - b1 * a12) / det
    n = np.cross(e1, e2)
    residual = np.abs((d * n).sum(1)) / np.linalg.norm(n, axis=1)
    return u, w, residual


# ---------------------------------------------------------------- 2. nearest point under a cutoff
def nearest(points, queries, max_distance, chunk=512):
    """(d2 f32[K], index u32[K]): brute force over all pairs in float32, the lowest index among equal d2; +inf and 0xFFFFFFFF without a candidate."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, F32).reshape(-1, 3)
    r = F32(max_distance)
    r2 = r * r
    K = q.shape[0]
    d2_out, idx_out = np.full(K, np.inf, F32), np.full(K, NO_INDEX, U32)
    usable = np.all(np.isfinite(p), axis=1)
    if p.shape[0] == 0 or K == 0:
        return d2_out, idx_out
    with np.errstate(all="ignore"):
        for s in range(0, K, chunk):
            c = q[s:s + chunk]
            dx, dy, dz = c[:, None, 0] - p[None, :, 0], c[:, None, 1] - p[None, :, 1], c[:, None, 2] - p[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            cand = (d2 <= r2) & usable[None, :]
            masked = np.where(cand, d2, F32(np.inf))
            best = np.argmin(masked, axis=1)           # the first, i.e. lowest, index of the minimum
            found = cand.any(axis=1)
            rows = np.arange(c.shape[0])
            d2_out[s:s + chunk] = np.where(found, masked[rows, best], F32(np.inf))
            idx_out[s:s + chunk] = np.where(found, best, NO_INDEX).astype(U32)
    return d2_out, idx_out


def nearest64(points, queries, chunk=512):
    """float64 brute force without a cutoff: (best d2, its index, second-best d2) per query over the finite points."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    usable = np.all(np.isfinite(p), axis=1)
    K = q.shape[0]
    best, idx, second = np.full(K, np.inf), np.full(K, -1, np.int64), np.full(K, np.inf)
    with np.errstate(all="ignore"):
        for s in range(0, K, chunk):
            d2 = ((q[s:s + chunk, None, :] - p[None, :, :]) ** 2).sum(axis=2)
            d2 = np.where(usable[None, :], d2, np.inf)
            if d2.shape[1] == 0:
                continue
            order = np.argsort(d2, axis=1, kind="stable")[:, :2]
            rows = np.arange(d2.shape[0])
            best[s:s + chunk], idx[s:s + chunk] = d2[rows, order[:, 0]], order[:, 0]
            if d2.shape[1] > 1:
                second[s:s + chunk] = d2[rows, order[:, 1]]
    return best, idx, second


# ---------------------------------------------------------------- 3. distance statistics
def distance_stats(d2, max_distance, threshold):
    """(n_found, n_within, sum_q) as Python ints."""
    d2 = np.ascontiguousarray(d2, F32).reshape(-1)
    r, t = F32(max_distance), F32(threshold)
    t2 = t * t
    found = np.isfinite(d2)
    with np.errstate(all="ignore"):
        x = (np.sqrt(d2[found]) / r) * F32(16777216.0)
    assert x.dtype == F32
    q = np.where(x > 0, np.minimum(x, F32(4294967296.0)), F32(0)).astype(np.int64)   # u32(f32): truncate, saturate
    q = np.minimum(q, 0xFFFFFFFF)
    return int(found.sum()), int((d2 <= t2).sum()), int(q.sum())


def direction(points, reference, max_distance, threshold):
    """points -> reference: dict(n, n_found, n_within, sum_q, mean)."""
    d2, _ = nearest(reference, points, max_distance)
    n_found, n_within, sum_q = distance_stats(d2, max_distance, threshold)
    mean = (sum_q * float(F32(max_distance)) / 2.0 ** 24 / n_found) if n_found else float("nan")
    return dict(n=int(d2.size), n_found=n_found, n_within=n_within, sum_q=sum_q, mean=mean)


def metrics_from(fwd, back):
    """The host arithmetic of geometryMetrics from the two directions' sums."""
    p = fwd["n_within"] / fwd["n"] if fwd["n"] else float("nan")
    r = back["n_within"] / back["n"] if back["n"] else float("nan")
    f = 0.0 if (p == 0 and r == 0) else 2 * p * r / (p + r)
    return dict(accuracy=fwd["mean"], completeness=back["mean"], chamfer=(fwd["mean"] + back["mean"]) / 2, precision=p, recall=r, fscore=f,
                n_points=fwd["n"], n_reference=back["n"], outliers_points=fwd["n"] - fwd["n_found"], outliers_reference=back["n"] - back["n_found"])


def geometry_metrics(points, reference, max_distance, threshold):
    return metrics_from(direction(points, reference, max_distance, threshold), direction(reference, points, max_distance, threshold))


# ---------------------------------------------------------------- shared shapes
def square_mesh(n, z=0.0, size=1.0):
    """The square [0, size]^2 at height z as 2 n^2 triangles: (vertices f32[(n+1)^2, 3], faces u32[2 n^2, 3])."""
    g = np.linspace(0.0, size, n + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], axis=1).astype(F32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    a = (j * (n + 1) + i).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + n + 2], axis=1), np.stack([a, a + n + 2, a + n + 1], axis=1)]).astype(U32)
    return v, f
