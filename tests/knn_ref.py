"""The k-nearest query and the neighbour-based scale initialisation of csrc/geometry.hip restated in numpy float32, operation for
operation: the GPU tests compare bytes.

``k_nearest`` is brute force over all pairs with ``geometry_ref.nearest``'s operation order, then a ``lexsort`` by (d2, index); it applies the cutoff, the
self-exclusion and the padding.  ``neighbour_scales`` is the per-point arithmetic of ``wdgs_point_cloud_neighbour_scales``.  ``k_nearest64`` is float64 and
serves only to check the restatement (tests/test_knn_reference.py)."""
import numpy as np

F32 = np.float32
U32 = np.uint32
NO_INDEX = 0xFFFFFFFF


def k_nearest(points, queries, k, max_distance, exclude_self=False, chunk=256):
    """(d2 f32[K, k], index u32[K, k]): per query the k first candidates by (d2, index); the rest +inf and 0xFFFFFFFF."""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, F32).reshape(-1, 3)
    r = F32(max_distance)
    r2 = r * r
    K, M = q.shape[0], p.shape[0]
    d2_out, idx_out = np.full((K, k), np.inf, F32), np.full((K, k), NO_INDEX, U32)
    usable = np.all(np.isfinite(p), axis=1)
    if M == 0 or K == 0:
        return d2_out, idx_out
    j = np.arange(M, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(0, K, chunk):
            c = q[s:s + chunk]
            dx, dy, dz = c[:, None, 0] - p[None, :, 0], c[:, None, 1] - p[None, :, 1], c[:, None, 2] - p[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            cand = (d2 <= r2) & usable[None, :] & np.all(np.isfinite(c), axis=1)[:, None]
            if exclude_self:
                cand &= j[None, :] != (s + np.arange(c.shape[0], dtype=np.int64))[:, None]
            for row in range(c.shape[0]):
                ids = j[cand[row]]
                dist = d2[row, cand[row]]
                order = np.lexsort((ids, dist))[:k]           # by d2, then by index
                d2_out[s + row, :order.size] = dist[order]
                idx_out[s + row, :order.size] = ids[order]
    return d2_out, idx_out


def k_nearest64(points, queries, k, exclude_self=False):
    """float64 brute force without a cutoff: the k + 1 smallest (d2 f64[K, k + 1], index i64[K, k + 1]) over the finite points, +inf / -1 padded."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    usable = np.all(np.isfinite(p), axis=1)
    K = q.shape[0]
    d2_out, idx_out = np.full((K, k + 1), np.inf), np.full((K, k + 1), -1, np.int64)
    if p.shape[0] == 0:
        return d2_out, idx_out
    with np.errstate(all="ignore"):
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    d2 = np.where(usable[None, :] & np.all(np.isfinite(q), axis=1)[:, None], d2, np.inf)
    if exclude_self:
        n = min(K, p.shape[0])
        d2[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")[:, :k + 1]
    got = np.take_along_axis(d2, order, axis=1)
    d2_out[:, :order.shape[1]] = got
    idx_out[:, :order.shape[1]] = np.where(np.isfinite(got), order, -1)
    return d2_out, idx_out


def f32_log(x, orc=None):
    """log in float32: the oracle's (bit-equal to the device's wd_log, tests/test_gpu_math.py) where given, else numpy's correctly rounded one."""
    x = np.ascontiguousarray(x, F32)
    if orc is None:
        with np.errstate(all="ignore"):
            return np.log(x.astype(np.float64)).astype(F32)
    import ctypes
    out = np.zeros(x.size, F32)
    orc.lib().orc_test_log(ctypes.c_uint32(x.size), x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(x.shape)


def neighbour_scales(gaussians, d2, min_d2=1e-7, orc=None):
    """(gaussians u32[N, 6] with halves 8, 9, 10 rewritten, meanD2 f32[N], found u32[N]) from k_nearest's d2 f32[N, k] of a self-query."""
    g = np.ascontiguousarray(gaussians, U32).reshape(-1, 6).copy()
    d2 = np.ascontiguousarray(d2, F32).reshape(g.shape[0], -1)
    finite = np.isfinite(d2)
    found = finite.sum(axis=1).astype(U32)
    s = np.zeros(g.shape[0], F32)
    for slot in range(d2.shape[1]):                       # slot order, from slot 0
        s = np.where(finite[:, slot], s + d2[:, slot], s)
    assert s.dtype == F32
    with np.errstate(all="ignore"):
        mean = np.where(found > 0, s / found.astype(F32), F32(np.inf)).astype(F32)
    m = np.maximum(mean, F32(min_d2))
    with np.errstate(over="ignore"):
        h = (F32(0.5) * f32_log(m, orc)).astype(np.float16).view(np.uint16)
    halves = g.view(np.uint16).reshape(-1, 12)
    has = found > 0
    for a in (8, 9, 10):
        halves[has, a] = h[has]
    return g, mean, found


def unpack_positions(gaussians):
    """f32[N, 3]: halves 0, 1, 2 of each record."""
    g = np.ascontiguousarray(gaussians, U32).reshape(-1, 6)
    return np.ascontiguousarray(g.view(np.float16).reshape(-1, 12)[:, :3].astype(F32))
