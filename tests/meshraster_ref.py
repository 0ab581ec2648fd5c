"""Mesh rasterization and depth agreement, restated: Python integers for the face classes and the edge functions' coefficients, int64
arrays over a face's bounding box for coverage (every value is below 2^48: exact), float32 arrays for depth and shading -- one numpy operation per rounding
of include/webdgs.h's definition, in its order -- and a loop over the faces.  ``rasterize`` returns every output and the statistics; ``CASES`` are the
crafted meshes the CPU and the GPU tests share; the cameras of the real-mesh cases come from tests/camzoo.py."""
import functools
import hashlib
import math

import numpy as np

from webdgs_amd import _lib

import camzoo
from meshsmooth_ref import icosphere

F32 = np.float32
NO_FACE = 0xFFFFFFFF
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
CULL = ("none", "back", "front")
STATS = ("invalidFaces", "clippedFaces", "degenerateFaces", "culledFaces", "emptyFaces", "rasterizedFaces", "coveredPixels", "viewportMismatch")
OUTPUTS = ("depth", "face", "colour", "normal")
T = _lib.MESH_RASTER_LARGE_FACE_PIXELS   # a bounding box of more pixels than this on either axis takes the other kernel: the cases straddle it
GUARD = 16384.0


# ---------------------------------------------------------------- the definition
def project(vertices, camera, W, H, near):
    """``(X, Y, view, usable)``: Python-int lists of the fixed-point positions (None where the vertex is not usable), the f32[V,3] view-space positions."""
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    c = np.ascontiguousarray(camera, F32).reshape(-1)
    with np.errstate(all="ignore"):
        v = np.stack([((c[0 + a] * p[:, 0] + c[4 + a] * p[:, 1]) + c[8 + a] * p[:, 2]) + c[12 + a] for a in range(3)], axis=1)
        z = v[:, 2]
        sx = (((c[32] * v[:, 0]) / z) * F32(0.5) + F32(0.5)) * F32(W)
        sy = ((((-c[37]) * v[:, 1]) / z) * F32(0.5) + F32(0.5)) * F32(H)
        assert v.dtype == sx.dtype == sy.dtype == F32
        usable = np.all(np.isfinite(v), axis=1) & (z >= F32(near)) & np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= F32(GUARD)) & (np.abs(sy) <= F32(GUARD))
        X = [int(np.rint(x * F32(256))) if u else None for x, u in zip(sx, usable)]
        Y = [int(np.rint(y * F32(256))) if u else None for y, u in zip(sy, usable)]
    return X, Y, v, usable


def _edges(X, Y, s):
    """Per edge k (from corner k + 1 to corner k + 2): ``(a, ex, ey, least)`` -- the start corner, the edge vector, and what a covered pixel's e_k is at least."""
    out = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        ex, ey = X[b] - X[a], Y[b] - Y[a]
        alpha, beta = -s * ey, s * ex
        owns = alpha > 0 or (alpha == 0 and beta > 0)
        out.append((a, ex, ey, 0 if owns else 1))
    return out


def _edge_values(X, Y, s, i, j):
    """The three e_k, int64 arrays, at the centres of the pixels ``(i, j)`` (int64 arrays), and the three ``least``."""
    cx, cy = 256 * i + 128, 256 * j + 128
    e, least = [], []
    for a, ex, ey, lo in _edges(X, Y, s):
        e.append(s * (ex * (cy - Y[a]) - ey * (cx - X[a])))
        least.append(lo)
    return e, least


def _depth(e, area, w):
    """``(lw, zp)``: the three rounded products lambda_k w_k and the depth, float32 arrays."""
    with np.errstate(all="ignore"):
        lw = [(ek.astype(F32) / F32(area)) * wk for ek, wk in zip(e, w)]
        zp = F32(1) / ((lw[0] + lw[1]) + lw[2])
    assert zp.dtype == F32
    return lw, zp


def _box(X, Y, W, H):
    i_lo, i_hi = max((min(X) + 127) >> 8, 0), min((max(X) - 128) >> 8, W - 1)
    j_lo, j_hi = max((min(Y) + 127) >> 8, 0), min((max(Y) - 128) >> 8, H - 1)
    return i_lo, i_hi, j_lo, j_hi


def rasterize(vertices, faces, colours, camera, width, height, near, cull="none"):
    """``dict(depth f32[H,W], face u32[H,W], colour u8[H,W,4] | None, normal f32[H,W,4], stats, large: the faces of the block kernel)``."""
    W, H = int(width), int(height)
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    cam = np.ascontiguousarray(camera, F32).reshape(-1)
    V = p.shape[0]
    X, Y, view, _ = project(p, cam, W, H, near)
    mismatch = not (cam[64] == F32(W) and cam[65] == F32(H))
    zbuf = np.full((H, W), EMPTY, np.uint64)
    counts = dict.fromkeys(STATS, 0)
    large = []
    with np.errstate(all="ignore"):
        inv_z = F32(1) / view[:, 2] if V else np.zeros(0, F32)
    corners = {}
    for n in range(f.shape[0]):
        c = [int(x) for x in f[n]]
        if any(x >= V for x in c):
            counts["invalidFaces"] += 1
            continue
        if any(X[x] is None for x in c):
            counts["clippedFaces"] += 1
            continue
        FX, FY = [X[x] for x in c], [Y[x] for x in c]
        A = (FX[1] - FX[0]) * (FY[2] - FY[0]) - (FX[2] - FX[0]) * (FY[1] - FY[0])
        if A == 0:
            counts["degenerateFaces"] += 1
            continue
        if (cull == "back" and A > 0) or (cull == "front" and A < 0):   # front is A < 0
            counts["culledFaces"] += 1
            continue
        i_lo, i_hi, j_lo, j_hi = _box(FX, FY, W, H)
        if i_lo > i_hi or j_lo > j_hi:
            counts["emptyFaces"] += 1
            continue
        counts["rasterizedFaces"] += 1
        if mismatch:
            continue
        if i_hi - i_lo >= T or j_hi - j_lo >= T:
            large.append(n)
        s = 1 if A > 0 else -1
        jj, ii = np.meshgrid(np.arange(j_lo, j_hi + 1, dtype=np.int64), np.arange(i_lo, i_hi + 1, dtype=np.int64), indexing="ij")
        e, least = _edge_values(FX, FY, s, ii, jj)
        assert all(abs(int(x)) < 2 ** 62 for ek in e for x in (ek.min(), ek.max()))
        assert np.array_equal(e[0] + e[1] + e[2], np.full(e[0].shape, abs(A)))
        inside = (e[0] >= least[0]) & (e[1] >= least[1]) & (e[2] >= least[2])
        _, zp = _depth(e, abs(A), [inv_z[x] for x in c])
        ok = inside & (zp > 0) & np.isfinite(zp)
        word = (zp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(n)
        sub = zbuf[j_lo:j_hi + 1, i_lo:i_hi + 1]
        sub[...] = np.where(ok, np.minimum(sub, word), sub)
        corners[n] = (c, FX, FY, s, abs(A))
    # ---- resolve
    hit = zbuf != EMPTY
    face = np.where(hit, zbuf & np.uint64(0xFFFFFFFF), np.uint64(NO_FACE)).astype(np.uint32)
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    normal = np.zeros((H, W, 4), F32)
    colour = None
    if colours is not None:
        colour = np.zeros((H, W, 4), np.uint8)
        col = np.ascontiguousarray(colours, np.uint8).reshape(V, -1)
    for n in sorted(set(int(x) for x in face[hit])):
        c, FX, FY, s, area = corners[n]
        mine = face == n
        jj, ii = np.nonzero(mine)
        if colour is not None:
            e, _ = _edge_values(FX, FY, s, ii.astype(np.int64), jj.astype(np.int64))
            lw, zp = _depth(e, area, [inv_z[x] for x in c])
            assert np.array_equal(zp.view(np.uint32), depth[mine].view(np.uint32))
            for ch in range(3):
                t = (lw[0] * F32(col[c[0], ch]) + lw[1] * F32(col[c[1], ch])) + lw[2] * F32(col[c[2], ch])
                x = t * zp
                x = np.where(x < 0, F32(0), x)          # max(x, 0) as the library's select: (x < 0) ? 0 : x
                x = np.where(F32(255) < x, F32(255), x)
                assert x.dtype == F32
                colour[jj, ii, ch] = np.rint(x).astype(np.uint8)
            colour[jj, ii, 3] = 255
        v0, v1, v2 = (view[x] for x in c)
        with np.errstate(all="ignore"):
            a, b = v1 - v0, v2 - v0
            g = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            nv = [x / length for x in g]
            assert all(isinstance(x, np.float32) for x in nv + [length])
            if (nv[0] * v0[0] + nv[1] * v0[1]) + nv[2] * v0[2] > 0:
                nv = [-x for x in nv]
        if all(np.isfinite(x) for x in nv) and any(x != 0 for x in nv):
            normal[jj, ii] = np.array(nv + [F32(1)], F32)
    counts["coveredPixels"] = int(hit.sum())
    counts["viewportMismatch"] = int(mismatch)
    return dict(depth=depth, face=face, colour=colour, normal=normal, stats=counts, large=large)


def depth_agreement(a, b, weight_sum, min_weight_sum, max_difference, threshold):
    """``[both, onlyA, onlyB, within, sum_q]`` as Python integers: a loop over the pixels, float32 scalars."""
    a, b = np.ascontiguousarray(a, F32).reshape(-1), np.ascontiguousarray(b, F32).reshape(-1)
    ws = None if weight_sum is None else np.ascontiguousarray(weight_sum, F32).reshape(-1)
    out = [0, 0, 0, 0, 0]
    md, th = F32(max_difference), F32(threshold)
    with np.errstate(all="ignore"):
        for k in range(a.size):
            has_a = bool(np.isfinite(a[k]) and a[k] > 0)
            has_b = bool(np.isfinite(b[k]) and b[k] > 0 and (ws is None or ws[k] >= F32(min_weight_sum)))
            if has_a and has_b:
                d = np.abs(a[k] - b[k])
                q = d / md
                q = F32(1) if F32(1) < q else q
                x = q * F32(16777216)
                assert isinstance(x, np.float32)
                out[0] += 1
                out[3] += int(d <= th)
                out[4] += int(x)
            elif has_a:
                out[1] += 1
            elif has_b:
                out[2] += 1
    return out


# ---------------------------------------------------------------- the crafted cases
def crafted_camera(W, H, block_size=None):
    """Identity view, P00 = P11 = 1: with power-of-two viewports a vertex placed by ``at`` lands exactly where it is put."""
    c = np.zeros(68, F32)
    c[[0, 5, 10, 15]] = 1
    c[32] = c[37] = 1
    c[64], c[65] = block_size or (W, H)
    return c


def at(sx, sy, z, W, H):
    """The world (= view) position that the crafted camera puts at pixel coordinates (sx, sy) and depth z."""
    return [(sx / W - 0.5) * 2.0 * z, -(sy / H - 0.5) * 2.0 * z, z]


def _case(vertices, faces, W, H, colours=None, camera=None, near=0.01, cull="none"):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    return dict(vertices=v, faces=np.ascontiguousarray(faces, np.uint32).reshape(-1, 3),
                colours=None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(v.shape[0], 4),
                camera=crafted_camera(W, H) if camera is None else np.ascontiguousarray(camera, F32), width=W, height=H, near=near, cull=cull)


def _rainbow(V, seed=0):
    c = np.random.default_rng(7000 + seed).integers(0, 256, (V, 4)).astype(np.uint8)
    c[:, 3] = 255
    return c


def _triangle_on_centres():
    W = H = 16
    v = [at(2.5, 2.5, 1.0, W, H), at(10.5, 2.5, 2.0, W, H), at(2.5, 10.5, 4.0, W, H)]
    return _case(v, [[0, 1, 2]], W, H, colours=[[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]])


def _split_quad(first, second, lo=1.0, hi=6.0, W=8, H=8):
    """A square whose diagonal from (lo, lo) to (hi, hi) runs through pixel centres, as two faces with the given corner orders."""
    def make():
        v = [at(lo, lo, 1.0, W, H), at(hi, lo, 1.0, W, H), at(hi, hi, 1.0, W, H), at(lo, hi, 1.0, W, H)]
        return _case(v, [first, second], W, H, colours=_rainbow(4))
    return make


def _fan(n, W, radius):
    """A closed fan of n faces round a hub on a pixel centre; the rim at alternating depths."""
    def make():
        hub = W / 2 + 0.5
        ang = np.arange(n) * (2 * math.pi / n) + 0.1
        v = [at(hub, hub, 2.0, W, W)] + [at(hub + radius * math.cos(t), hub + radius * math.sin(t), 2.0 + 0.5 * (k % 2), W, W) for k, t in enumerate(ang)]
        return _case(v, [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], W, W, colours=_rainbow(n + 1, n))
    return make


def _identical_pair(swapped):
    def make():
        W = H = 16
        tri = [at(1.0, 1.0, 2.0, W, H), at(14.0, 2.0, 2.0, W, H), at(3.0, 13.0, 3.0, W, H)]
        faces = [[0, 1, 2], [3, 4, 5]]
        return _case(tri + tri, faces[::-1] if swapped else faces, W, H, colours=[[255, 0, 0, 255]] * 3 + [[0, 0, 255, 255]] * 3)
    return make


def _intersecting():
    W = H = 32
    v = [at(2, 2, 1.0, W, H), at(30, 3, 3.0, W, H), at(4, 29, 2.0, W, H), at(3, 3, 3.0, W, H), at(29, 2, 1.0, W, H), at(28, 30, 2.0, W, H)]
    return _case(v, [[0, 1, 2], [3, 4, 5]], W, H, colours=_rainbow(6, 1))


def _stack(front_to_back):
    def make():
        W = H = 32
        v, f = [], []
        layers = list(range(6))
        for k in (layers if front_to_back else layers[::-1]):
            z = 1.0 + 0.25 * k
            f.append([len(v), len(v) + 1, len(v) + 2])
            v += [at(3.0 + k, 2.0, z, W, H), at(29.0, 4.0 + k, z, W, H), at(5.0, 30.0 - k, z, W, H)]
        return _case(v, f, W, H)
    return make


def _classes():
    """One face or more of every class; EXPECT holds the counts."""
    W = H = 64
    nan, inf = float("nan"), float("inf")
    v, f = [], []

    def tri(a, b, c):
        f.append([len(v), len(v) + 1, len(v) + 2])
        v.extend([a, b, c])

    tri(at(5, 5, 2.0, W, H), at(20, 6, 2.0, W, H), at(6, 21, 2.0, W, H))                    # rasterized
    tri([0.0, 0.0, 0.005], [0.001, 0.0, 0.005], [0.0, 0.001, 0.005])                       # behind near (0.01): clipped
    tri(at(30, 30, 1.0, W, H), at(40, 30, 1.0, W, H), [0.0, 0.1, 0.004])                    # straddles near: clipped
    tri(at(30, 30, 1.0, W, H), at(40, 30, 1.0, W, H), [0.0, 0.1, -1.0])                     # a vertex behind the camera: clipped
    tri(at(30, 30, 1.0, W, H), at(40, 30, 1.0, W, H), [600.0, 0.0, 1.0])                    # sx = 19232 > 16384: clipped
    tri(at(30, 30, 1.0, W, H), at(40, 30, 1.0, W, H), [0.0, -600.0, 1.0])                   # sy beyond the guard band: clipped
    tri(at(30, 30, 1.0, W, H), [nan, 0.0, 1.0], at(40, 40, 1.0, W, H))                      # NaN: clipped
    tri(at(30, 30, 1.0, W, H), [0.0, inf, 1.0], at(40, 40, 1.0, W, H))                      # inf: clipped
    tri(at(30, 30, 1.0, W, H), at(40, 40, 1.0, W, H), [0.0, 0.0, inf])                      # z = inf: clipped
    f.append([0, 1, 1000000])                                                              # an index >= V: invalid
    f.append([NO_FACE, 0, 1])                                                              # invalid
    f.append([0, 2 ** 31, 1])                                                              # invalid
    tri(at(50.0, 50.0, 1.0, W, H), at(50.0 + 1 / 1024, 50.0, 1.0, W, H), at(50.0, 50.0 + 1 / 1024, 1.0, W, H))   # snaps to one point: degenerate
    tri(at(10, 40, 1.0, W, H), at(20, 40, 1.0, W, H), at(30, 40 + 1 / 1024, 1.0, W, H))     # snaps to a line: degenerate
    tri(at(45.6, 45.6, 1.0, W, H), at(46.4, 45.6, 1.0, W, H), at(45.6, 46.4, 1.0, W, H))     # between pixel centres: empty
    tri(at(40.1, 10.6, 1.0, W, H), at(44.9, 10.7, 1.0, W, H), at(40.2, 11.4, 1.0, W, H))     # a box without a centre row: empty
    tri(at(-30, 10, 1.0, W, H), at(-5, 12, 1.0, W, H), at(-20, 30, 1.0, W, H))              # wholly left: empty
    tri(at(70, 10, 1.0, W, H), at(95, 12, 1.0, W, H), at(80, 30, 1.0, W, H))                # wholly right: empty
    tri(at(10, -30, 1.0, W, H), at(30, -5, 1.0, W, H), at(12, -20, 1.0, W, H))              # wholly above: empty
    tri(at(10, 70, 1.0, W, H), at(30, 95, 1.0, W, H), at(12, 80, 1.0, W, H))                # wholly below: empty
    tri(at(-6, 30, 1.5, W, H), at(5, 28, 1.5, W, H), at(2, 40, 1.5, W, H))                  # clamped by the left side: rasterized
    tri(at(58, 30, 1.5, W, H), at(75, 28, 1.5, W, H), at(60, 45, 1.5, W, H))                # clamped by the right side (a large face)
    tri(at(30, -8, 1.5, W, H), at(44, -2, 1.5, W, H), at(36, 6, 1.5, W, H))                 # clamped by the top
    tri(at(30, 70, 1.5, W, H), at(50, 60, 1.5, W, H), at(33, 58, 1.5, W, H))                # clamped by the bottom (a large face)
    tri(at(8.1, 50.3, 1.0, W, H), at(8.9, 51.1, 1.0, W, H), at(8.15, 50.3, 1.0, W, H))       # a sliver whose box holds the centre (8.5, 50.5) and that misses it: rasterized
    return _case(v, f, W, H, colours=_rainbow(len(v), 2))


def _threshold(extent, axis):
    """A right triangle whose bounding box holds exactly ``extent`` pixel centres along ``axis`` and 5 along the other."""
    def make():
        W = H = 64
        lo = 3.25
        long, short = lo + extent - 0.5, lo + 4.5      # centres lo + 0.25 .. : extent (or 5) of them
        far = (long, lo) if axis == 0 else (lo, long)
        near_ = (lo, short) if axis == 0 else (short, lo)
        v = [at(lo, lo, 1.0, W, H), at(far[0], far[1], 2.0, W, H), at(near_[0], near_[1], 1.5, W, H)]
        return _case(v, [[0, 1, 2]], W, H, colours=_rainbow(3, extent))
    return make


def _mixed():
    """Two faces that fill the viewport behind a thousand small ones, at 67 x 45: both kernels into one image, the viewport no multiple of a block."""
    W, H = 67, 45
    rng = np.random.default_rng(41)
    v = [at(-5, -5, 6.0, W, H), at(80, -5, 6.0, W, H), at(80, 60, 6.5, W, H), at(-5, 60, 6.5, W, H)]
    f = [[0, 1, 2], [0, 2, 3]]
    for _ in range(1000):
        cx, cy, z = rng.uniform(-2, W + 2), rng.uniform(-2, H + 2), rng.uniform(1.0, 5.0)
        d = rng.uniform(-3.0, 3.0, (3, 2))
        f.append([len(v), len(v) + 1, len(v) + 2])
        v += [at(cx + d[k, 0], cy + d[k, 1], z + 0.1 * k, W, H) for k in range(3)]
    return _case(v, f, W, H, colours=_rainbow(len(v), 3))


def _layers(n, W, H):
    """n faces that each fill the viewport.  40 at 128 x 128: 40 x 256 work items, more than the block kernel's grid has waves (8 workgroups of 4 on each of 256
    CUs), so a wave's run is two items.  45 at 120 x 104: 45 x 195 items, again two a wave, and a face's odd count puts the start of a face inside a run."""
    def make():
        return _layers_case(n, W, H)
    return make


def _layers_case(n, W, H):
    v, f = [], []
    for k in range(n):
        z = 2.0 + 0.05 * ((k * 17) % n)
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
        v += [at(-10, -10, z, W, H), at(300, -10, z, W, H), at(-10, 300, z + 0.5, W, H)]
    return _case(v, f, W, H, colours=_rainbow(len(v), 4))


def _sphere(camera_name, cull="none", radius=1.5):
    def make():
        W, H = camzoo.ZOO_CFG.width, camzoo.ZOO_CFG.height
        v, f = icosphere(2)
        position, target, _, _ = camzoo.poses()[camera_name]
        if camera_name == "close":   # the zoo's scene is not where this camera looks: a sphere the camera stands just outside of
            d = np.asarray(target, np.float64) - np.asarray(position, np.float64)
            centre, r = np.asarray(position, np.float64) + 1.05 * d / np.linalg.norm(d), 1.0
        else:
            centre, r = np.array([0.0, 0.0, 6.0]), radius
        return _case(v * r + centre, f, W, H, colours=_rainbow(v.shape[0], 5), camera=camzoo.camera(camera_name), cull=cull)
    return make


def _mismatch():
    W = H = 16
    m = _triangle_on_centres()
    return dict(m, camera=crafted_camera(W, H, block_size=(32, 32)))


CASES = {
    "nothing": lambda: _case(np.zeros((0, 3)), np.zeros((0, 3)), 8, 8),
    "no-faces": lambda: _case([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.zeros((0, 3)), 8, 8, colours=_rainbow(3)),
    "no-vertices": lambda: _case(np.zeros((0, 3)), [[0, 1, 2]], 8, 8),
    "one-pixel": lambda: _case([at(-1, -1, 1.0, 1, 1), at(3, -1, 1.0, 1, 1), at(-1, 3, 1.0, 1, 1)], [[0, 1, 2]], 1, 1, colours=_rainbow(3)),
    "triangle-on-centres": _triangle_on_centres,
    # the diagonal's pixels belong to exactly one of the two faces whichever way each is wound
    "split-quad-ccw-ccw": _split_quad([0, 1, 2], [0, 2, 3]), "split-quad-ccw-cw": _split_quad([0, 1, 2], [0, 3, 2]), "split-quad-cw-cw": _split_quad([2, 1, 0], [3, 2, 0]),
    "split-quad-large": _split_quad([0, 1, 2], [0, 2, 3], lo=3.0, hi=43.0, W=64, H=64),
    "fan-16": _fan(16, 32, 0.7 * T), "fan-65": _fan(65, 64, 27.7), "fan-16-large": _fan(16, 128, 55.1),
    "identical-pair": _identical_pair(False), "identical-pair-swapped": _identical_pair(True),
    "intersecting": _intersecting,
    "stack-front-to-back": _stack(True), "stack-back-to-front": _stack(False),
    "classes": _classes,
    "threshold-at-x": _threshold(T, 0), "threshold-above-x": _threshold(T + 1, 0), "threshold-at-y": _threshold(T, 1), "threshold-above-y": _threshold(T + 1, 1),
    "mixed-67x45": _mixed,
    "forty-layers": _layers(40, 128, 128), "layers-120x104": _layers(45, 120, 104),
    "sphere-roll37": _sphere("roll37"), "sphere-roll37-back": _sphere("roll37", "back"), "sphere-roll37-front": _sphere("roll37", "front"),
    "sphere-below": _sphere("below"), "sphere-close": _sphere("close"),
    "viewport-mismatch": _mismatch,
}
# what the definition gives, where the case is about it
EXPECT = {
    "nothing": dict(coveredPixels=0, rasterizedFaces=0), "no-faces": dict(coveredPixels=0), "no-vertices": dict(invalidFaces=1, coveredPixels=0),
    "one-pixel": dict(rasterizedFaces=1, coveredPixels=1),
    "triangle-on-centres": dict(rasterizedFaces=1, coveredPixels=36),   # rows of 8, 7, .. 1 centres on or inside, less those on the edges it does not own
    "split-quad-ccw-ccw": dict(coveredPixels=25), "split-quad-ccw-cw": dict(coveredPixels=25), "split-quad-cw-cw": dict(coveredPixels=25),
    "split-quad-large": dict(coveredPixels=1600),
    "classes": dict(invalidFaces=3, clippedFaces=8, degenerateFaces=2, emptyFaces=6, culledFaces=0, rasterizedFaces=6),
    "threshold-at-x": dict(rasterizedFaces=1), "threshold-above-x": dict(rasterizedFaces=1),
    "forty-layers": dict(rasterizedFaces=40, coveredPixels=128 * 128), "layers-120x104": dict(rasterizedFaces=45, coveredPixels=120 * 104),
    "mixed-67x45": dict(coveredPixels=67 * 45),
    "viewport-mismatch": dict(rasterizedFaces=1, coveredPixels=0, viewportMismatch=1),
}
# the number of faces the block kernel draws, where the case is about the path taken
EXPECT_LARGE = {"threshold-at-x": 0, "threshold-above-x": 1, "threshold-at-y": 0, "threshold-above-y": 1, "forty-layers": 40, "layers-120x104": 45, "split-quad-large": 2, "fan-16": 0,
                "fan-16-large": 16}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name: ``dict(vertices, faces, colours | None, camera, width, height, near, cull)``; computed once and shared: callers leave it unchanged."""
    m = CASES[name]()
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name):
    """``rasterize`` of that case; computed once and shared: callers leave it unchanged."""
    m = case(name)
    out = rasterize(m["vertices"], m["faces"], m["colours"], m["camera"], m["width"], m["height"], m["near"], m["cull"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def digest(result):
    """sha256 over the result's images in a fixed order (a missing colour image is skipped), then its statistics (what a host's run script prints)."""
    h = hashlib.sha256()
    for k in OUTPUTS:
        if result.get(k) is not None:
            h.update(np.ascontiguousarray(result[k]).tobytes())
    h.update(np.array([result["stats"][k] for k in STATS], np.uint32).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- depth agreement: crafted image pairs
def _agreement_cases():
    nan, inf = float("nan"), float("inf")
    md, th = 0.5, 0.125
    a = np.array([1.0, 1.0, 0.0, 2.0, 2.0, 2.0, nan, 1.0, -1.0, 1.0, inf, 3.0, 1.0, 0.0, 5.0, 1.0], F32)
    b = np.array([1.0, 0.0, 1.0, 2.125, 2.5, 3.5, 1.0, nan, 1.0, -2.0, 1.0, inf, 1.0625, 0.0, 5.13, 1.0], F32)
    ws = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.25, 1.0, 0.5, nan], F32)
    rng = np.random.default_rng(9)
    ra = rng.uniform(0.5, 4.0, 67 * 45).astype(F32)
    rb = (ra + rng.normal(0.0, 0.2, ra.size)).astype(F32)
    ra[rng.integers(0, ra.size, 300)] = 0
    rb[rng.integers(0, ra.size, 300)] = 0
    rw = rng.uniform(0.0, 1.0, ra.size).astype(F32)
    return {
        "crafted": dict(a=a, b=b, weight_sum=None, min_weight_sum=0.0, width=16, height=1, max_difference=md, threshold=th),
        "crafted-masked": dict(a=a, b=b, weight_sum=ws, min_weight_sum=0.5, width=4, height=4, max_difference=md, threshold=th),
        "a-absent": dict(a=np.zeros(12, F32), b=np.full(12, 2.0, F32), weight_sum=None, min_weight_sum=0.0, width=4, height=3, max_difference=1.0, threshold=1.0),
        "b-absent": dict(a=np.full(12, 2.0, F32), b=np.zeros(12, F32), weight_sum=None, min_weight_sum=0.0, width=3, height=4, max_difference=1.0, threshold=0.5),
        "random-67x45": dict(a=ra, b=rb, weight_sum=rw, min_weight_sum=0.3, width=67, height=45, max_difference=0.25, threshold=0.1),
    }


AGREEMENT_CASES = _agreement_cases()
# crafted: d = 0 | - | - | 0.125 = threshold | 0.5 = max_difference | 1.5 > max | ... | 0.0625 | - | 0.13 | 0
AGREEMENT_EXPECT = {"a-absent": [0, 0, 12, 0, 0], "b-absent": [0, 12, 0, 0, 0]}


def agreement_expected(name):
    c = AGREEMENT_CASES[name]
    return depth_agreement(c["a"], c["b"], c["weight_sum"], c["min_weight_sum"], c["max_difference"], c["threshold"])
