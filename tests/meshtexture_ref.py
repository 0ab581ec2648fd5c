"""A texture atlas baked from photographs, restated: numpy float32 arrays over the texels -- one numpy operation per rounding of
include/webdgs.h's definition, in its order -- for the face, the texel's point and the weight, integer arrays for everything else.  ``layout`` and ``texels``
are the atlas, ``accumulate`` adds one view to a state, ``resolve`` turns a state into a texture; ``CASES`` are the crafted meshes and views the CPU and the
GPU tests share."""
import functools
import hashlib
import math

import numpy as np

import camzoo
import meshraster_ref as mr
from meshraster_ref import at, crafted_camera

F32 = np.float32
STATS = ("invalidFaces", "facingAwayFaces", "offImageFaces", "usable", "inImage", "visible", "accumulated", "viewportMismatch", "bakedTexels", "filledTexels",
         "fallbackTexels")
CELLS = (4, 8, 16, 32)
NEAR = 0.01
MAX_SIZE = 16384
MAX_ACCUMULATES = 65535


# ---------------------------------------------------------------- the atlas
def layout(F, C):
    """``dict(width, height, cellsPerRow, cells, rows, uv f32[F,3,2])``."""
    assert C in CELLS and 0 <= F < 2 ** 31
    cells = (F + 1) // 2
    per_row = math.isqrt(cells)
    if per_row * per_row < cells:
        per_row += 1
    rows = -(-cells // per_row) if per_row else 0
    Wt, Ht = per_row * C, rows * C
    assert Wt <= MAX_SIZE
    m = C - 3
    uv = np.zeros((F, 3, 2), F32)
    for f in range(F):
        k, odd = f // 2, f % 2
        for c, (ip, jp) in enumerate(((0, 0), (m, 0), (0, m))):
            i, j = (C - 1 - ip, C - 1 - jp) if odd else (ip, jp)
            x, y = (k % per_row) * C + i, (k // per_row) * C + j
            uv[f, c] = [(x + 0.5) / Wt, 1.0 - (y + 0.5) / Ht]
    return dict(width=Wt, height=Ht, cellsPerRow=per_row, cells=cells, rows=rows, uv=uv)


def owner(i, j, C):
    """0: the even face of the cell, 1: the odd one, -1: nobody."""
    s = i + j
    return 0 if s <= C - 2 else (1 if s >= C else -1)


@functools.lru_cache(maxsize=None)
def texels(F, C):
    """Every owned texel of the atlas of ``F`` faces, int64 arrays: ``row`` (its place in the cell-major state), ``face``, ``ip``, ``jp`` (its place in
    the face's chart), ``x``, ``y`` (its place in the atlas).  Shared: callers leave it unchanged."""
    L = layout(F, C)
    cell, j, i = np.meshgrid(np.arange(L["cells"]), np.arange(C), np.arange(C), indexing="ij")
    s = i + j
    odd = s >= C
    face = 2 * cell + odd
    keep = (s != C - 1) & (face < F)
    out = dict(row=(cell * C * C + j * C + i)[keep], face=face[keep], ip=np.where(odd, C - 1 - i, i)[keep], jp=np.where(odd, C - 1 - j, j)[keep],
               x=((cell % max(L["cellsPerRow"], 1)) * C + i)[keep], y=((cell // max(L["cellsPerRow"], 1)) * C + j)[keep])
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the definition
def new_state(F, C, accumulates=0):
    """The state after ``reset(F, C)``."""
    return dict(F=int(F), C=int(C), rows=np.zeros((((F + 1) // 2) * C * C, 4), np.int64), totals=dict.fromkeys(STATS, 0), accumulates=accumulates)


def _view_space(p, c):
    return [((c[0 + a] * p[..., 0] + c[4 + a] * p[..., 1]) + c[8 + a] * p[..., 2]) + c[12 + a] for a in range(3)]


def _screen(x, y, z, c, W, H):
    sx = (((c[32] * x) / z) * F32(0.5) + F32(0.5)) * F32(W)
    sy = ((((-c[37]) * y) / z) * F32(0.5) + F32(0.5)) * F32(H)
    assert sx.dtype == sy.dtype == F32
    return sx, sy


def _Q(n, nn, p, min_cos, two_sided):
    """Step 1's Q for points ``p`` (three f32 arrays) of faces with normals ``n`` (three f32 arrays): an int64 array."""
    dot = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
    pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    c = (-dot) / np.sqrt(nn * pp)
    assert c.dtype == F32
    if two_sided:
        c = np.abs(c)
    ok = np.isfinite(c) & ~(c < F32(min_cos))
    q = np.rint(np.where(c > F32(1), F32(1), c) * F32(256))
    return np.where(ok, np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)


def classify(vertices, faces, cam, W, H, near, min_cos, two_sided):
    """Step 1: ``(P, n, nn, cls)`` -- the corners in view space as ``P[k][a]`` f32[F], the normal, and the class of every face: 0 live, 1 invalid, 2 facing
    away, 3 off the image."""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    V = v.shape[0]
    in_range = f < V
    g = np.where(in_range, f, 0)
    corners = v[g] if V else np.zeros(f.shape + (3,), F32)   # [F, 3, 3]
    P = [_view_space(corners[:, k], cam) for k in range(3)]
    good = [in_range[:, k] & np.isfinite(P[k][0]) & np.isfinite(P[k][1]) & np.isfinite(P[k][2]) & (P[k][2] >= F32(near)) for k in range(3)]
    invalid = ~(good[0] & good[1] & good[2])
    a = [P[1][i] - P[0][i] for i in range(3)]
    b = [P[2][i] - P[0][i] for i in range(3)]
    n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    away = np.ones(f.shape[0], bool)
    sides = [np.ones(f.shape[0], bool) for _ in range(4)]
    for k in range(3):
        away &= _Q(n, nn, P[k], min_cos, two_sided) == 0
        sx, sy = _screen(P[k][0], P[k][1], P[k][2], cam, W, H)
        for s, test in zip(sides, (sx < F32(0), sx > F32(W), sy < F32(0), sy > F32(H))):
            s &= test
    off = sides[0] | sides[1] | sides[2] | sides[3]
    cls = np.where(invalid, 1, np.where(away, 2, np.where(off, 3, 0)))
    return P, n, nn, cls


def accumulate(state, vertices, faces, camera, image, depth, width, height, near=NEAR, depth_tolerance=0.0625, min_cos=0.0, two_sided=False):
    """One view added to ``state``, in place."""
    W, H, C = int(width), int(height), state["C"]
    cam = np.ascontiguousarray(camera, F32).reshape(-1)
    t = state["totals"]
    assert state["accumulates"] < MAX_ACCUMULATES
    state["accumulates"] += 1
    if not (cam[64] == F32(W) and cam[65] == F32(H)):
        t["viewportMismatch"] += 1
        return state
    F = state["F"]
    assert np.asarray(faces).reshape(-1, 3).shape[0] == F
    img = np.ascontiguousarray(image, np.uint8).reshape(H, W, 4).astype(np.int64)
    dep = None if depth is None else np.ascontiguousarray(depth, F32).reshape(H, W)
    with np.errstate(all="ignore"):
        P, n, nn, cls = classify(vertices, faces, cam, W, H, near, min_cos, two_sided)
        for k, name in ((1, "invalidFaces"), (2, "facingAwayFaces"), (3, "offImageFaces")):
            t[name] += int((cls == k).sum())
        tx = texels(F, C)
        sel = cls[tx["face"]] == 0
        row, face = tx["row"][sel], tx["face"][sel]
        m = F32(C - 3)
        u, v = tx["ip"][sel].astype(F32) / m, tx["jp"][sel].astype(F32) / m
        w = (F32(1) - u) - v
        p = [(w * P[0][a][face] + u * P[1][a][face]) + v * P[2][a][face] for a in range(3)]
        sx, sy = _screen(p[0], p[1], p[2], cam, W, H)
        usable = (np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2]) & (p[2] >= F32(near)) & np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= F32(mr.GUARD))
                  & (np.abs(sy) <= F32(mr.GUARD)))
        t["usable"] += int(usable.sum())
        keep = np.flatnonzero(usable)
        X = np.rint(sx[keep] * F32(256)).astype(np.int64) - 128
        Y = np.rint(sy[keep] * F32(256)).astype(np.int64) - 128
        inside = (X >= 0) & (X <= 256 * (W - 1)) & (Y >= 0) & (Y <= 256 * (H - 1))
        t["inImage"] += int(inside.sum())
        keep, X, Y = keep[inside], X[inside], Y[inside]
        i0, a, j0, b = X >> 8, X & 255, Y >> 8, Y & 255
        i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
        if dep is not None:
            z = p[2][keep]
            seen = np.ones(keep.shape[0], bool)
            for jj, ii in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)):
                d = dep[jj, ii]
                seen &= np.isfinite(d) & (d > 0) & (np.abs(z - d) <= F32(depth_tolerance))
            keep, i0, i1, j0, j1, a, b = (x[seen] for x in (keep, i0, i1, j0, j1, a, b))
        t["visible"] += int(keep.shape[0])
        fk = face[keep]
        Q = _Q([c[fk] for c in n], nn[fk], [c[keep] for c in p], min_cos, two_sided)
        on = Q != 0
        t["accumulated"] += int(on.sum())
        keep, i0, i1, j0, j1, a, b, Q = (x[on] for x in (keep, i0, i1, j0, j1, a, b, Q))
    S = ((256 - a) * (256 - b))[:, None] * img[j0, i0, :3] + (a * (256 - b))[:, None] * img[j0, i1, :3] + ((256 - a) * b)[:, None] * img[j1, i0, :3] \
        + (a * b)[:, None] * img[j1, i1, :3]
    s = (S + 32768) >> 16
    assert s.size == 0 or s.max() <= 255
    r = row[keep]
    state["rows"][r, :3] += Q[:, None] * s   # (a texel appears once: no repeated index)
    state["rows"][r, 3] += Q
    assert state["rows"].max(initial=0) < 2 ** 32
    return state


def _baked_colour(rows):
    Wsum = np.maximum(rows[:, 3:4], 1)
    return np.minimum((rows[:, :3] + Wsum // 2) // Wsum, 255)


def resolve(state, faces, colours=None, num_vertices=0, min_weight=1, fill=True):
    """``(texture u8[Ht,Wt,4], texelState u8[Ht,Wt])``, and the three texel totals of the state set."""
    F, C = state["F"], state["C"]
    L = layout(F, C)
    texture, tstate = np.zeros((L["height"], L["width"], 4), np.uint8), np.zeros((L["height"], L["width"]), np.uint8)
    tx = texels(F, C)
    rows = state["rows"]
    threshold = max(int(min_weight), 1)
    baked_all = rows[:, 3] >= threshold                    # by row; rows nobody owns are zero
    colour_all = _baked_colour(rows)
    n_rows = rows.shape[0]
    # the owner of every row: the face, or -1
    owner_all = np.full(n_rows, -1, np.int64)
    owner_all[tx["row"]] = tx["face"]
    row, face = tx["row"], tx["face"]
    baked = baked_all[row]
    out = np.zeros((row.shape[0], 3), np.int64)
    out[baked] = colour_all[row[baked]]
    st = np.where(baked, 1, 0)
    local = row % (C * C)
    i, j = local % C, local // C
    total, count = np.zeros((row.shape[0], 3), np.int64), np.zeros(row.shape[0], np.int64)
    if fill:
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if di == 0 and dj == 0:
                    continue
                ok = (i + di >= 0) & (i + di < C) & (j + dj >= 0) & (j + dj < C)
                other = np.where(ok, row + dj * C + di, 0)
                ok &= (owner_all[other] == face) & baked_all[other]
                total[ok] += colour_all[other[ok]]
                count[ok] += 1
    filled = ~baked & (count > 0)
    cnt = np.maximum(count, 1)[:, None]
    out[filled] = ((total + cnt // 2) // cnt)[filled]
    st[filled] = 2
    rest = ~baked & ~filled
    m = C - 3
    i2 = np.minimum(tx["ip"], m)
    j2 = np.minimum(tx["jp"], m - i2)
    k2 = m - i2 - j2
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    V = int(num_vertices)
    c = np.zeros((F, 3, 3), np.int64)
    if colours is not None and F:
        col = np.ascontiguousarray(colours, np.uint8).reshape(V, 4).astype(np.int64)
        ok = f < V
        c = np.where(ok[:, :, None], col[np.where(ok, f, 0), :3] if V else 0, 0)
    fb = (k2[:, None] * c[face, 0] + i2[:, None] * c[face, 1] + j2[:, None] * c[face, 2] + m // 2) // m if F else out
    out[rest] = fb[rest]
    texture[tx["y"], tx["x"], :3] = out
    texture[tx["y"], tx["x"], 3] = 255
    tstate[tx["y"], tx["x"]] = st
    state["totals"].update(bakedTexels=int(baked.sum()), filledTexels=int(filled.sum()), fallbackTexels=int(rest.sum()))
    return texture, tstate


# ---------------------------------------------------------------- the crafted cases
# A case: dict(vertices f32[V,3], faces u32[F,3], colours u8[V,4] | None, cell, views: [dict(camera, image u8[H,W,4], depth f32[H,W] | None | "mesh", width,
# height, near, depth_tolerance, min_cos, two_sided)], min_weight, fill).  A depth of "mesh" is the mesh's own depth image, from ``meshraster_ref.rasterize``.
def _view(image, depth=None, camera=None, near=NEAR, depth_tolerance=0.0625, min_cos=0.0, two_sided=False):
    image = np.ascontiguousarray(image, np.uint8)
    H, W = image.shape[:2]
    return dict(camera=crafted_camera(W, H) if camera is None else np.ascontiguousarray(camera, F32), image=image, depth=depth, width=W, height=H, near=near,
                depth_tolerance=depth_tolerance, min_cos=min_cos, two_sided=two_sided)


def _case(vertices, faces, views, cell=8, colours=None, min_weight=1, fill=True):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    return dict(vertices=v, faces=np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), cell=cell, views=views,
                colours=None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(v.shape[0], 4), min_weight=min_weight, fill=fill)


def noise_image(W, H, seed):
    return np.random.default_rng(9000 + seed).integers(0, 256, (H, W, 4)).astype(np.uint8)


def ramp_image(W, H):
    """T(i, j) = 3 i + 2 j in red, 255 - that in green, j in blue: at most 3 levels a pixel."""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = 3 * i + 2 * j
    assert t.max() <= 255
    return np.stack([t, 255 - t, j, np.full_like(t, 77)], axis=2).astype(np.uint8)


def _tiles(F, W, H, seed, z=2.0, jitter=0.0):
    """F faces, each a small triangle of its own (three vertices each) that faces the camera, scattered over a W x H image at depths round z."""
    rng = np.random.default_rng(300 + seed)
    v, f = [], []
    for k in range(F):
        cx, cy = rng.uniform(2, W - 2), rng.uniform(2, H - 2)
        size = rng.uniform(1.5, 6.0)
        zz = z + rng.uniform(-jitter, jitter)
        # (v1 to the right of v0 and v2 below it on the screen: (v1 - v0) x (v2 - v0) points to the camera)
        v += [at(cx, cy, zz, W, H), at(cx + size, cy, zz + rng.uniform(-jitter, jitter), W, H), at(cx, cy + size, zz + rng.uniform(-jitter, jitter), W, H)]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.array(v, F32).reshape(-1, 3), np.array(f, np.uint32).reshape(-1, 3)


def _counts(F, C, seed):
    """F scattered faces in cells of C: two noise views, the second with the mesh's own depth image."""
    def make():
        W, H = 37, 29
        v, f = _tiles(F, W, H, seed, jitter=0.2)
        views = [_view(noise_image(W, H, seed), min_cos=0.1), _view(noise_image(W, H, seed + 1), depth="mesh", min_cos=0.0)]
        return _case(v, f, views, cell=C, colours=mr._rainbow(v.shape[0], 20 + seed))
    return make


def _quad(W, H, z=2.0, x0=4.0, y0=3.0, x1=None, y1=None):
    """A fronto-parallel quad of two faces that face the camera, from pixel (x0, y0) to (x1, y1)."""
    x1, y1 = W - 4.0 if x1 is None else x1, H - 3.0 if y1 is None else y1
    v = [at(x0, y0, z, W, H), at(x0, y1, z, W, H), at(x1, y0, z, W, H), at(x1, y1, z, W, H)]
    return np.array(v, F32), np.array([[0, 2, 1], [3, 1, 2]], np.uint32)


def _geometry(C):
    """One mesh of faces that each meet one face-level or texel-level rule, under one view with the mesh's own depth image; then the same without the
    occlusion test and two-sided."""
    def make():
        W, H = 64, 48
        nan = float("nan")
        v = [
            # 0: behind near; 1: crossing near
            at(10, 10, 0.001, W, H), at(10, 20, 0.001, W, H), at(20, 10, 0.001, W, H),
            at(30, 10, 1.0, W, H), at(30, 20, 0.005, W, H), at(40, 10, 1.0, W, H),
            # 2: half outside the image (to the left)
            at(-9, 24, 2.0, W, H), at(-9, 40, 2.0, W, H), at(9, 24, 2.0, W, H),
            # 3: back-facing (the other winding: the face list below swaps two corners)
            at(44, 30, 2.0, W, H), at(56, 30, 2.0, W, H), at(44, 42, 2.0, W, H),
            # 4: hidden by 5, which lies in front of it
            at(20, 26, 3.0, W, H), at(20, 40, 3.0, W, H), at(36, 26, 3.0, W, H),
            at(18, 24, 1.5, W, H), at(18, 44, 1.5, W, H), at(40, 24, 1.5, W, H),
            # 6: zero area (a corner twice); 7: an index >= V (below); 8: a NaN vertex
            at(50, 5, 2.0, W, H), at(55, 10, 2.0, W, H), at(60, 15, 2.0, W, H),
            at(5, 5, 2.0, W, H), at(5, 9, 2.0, W, H),
            [nan, 0.0, 2.0], at(50, 20, 2.0, W, H), at(54, 20, 2.0, W, H),
            # 9: wholly off the image, to the right; 10: grazing, steeper than min_cos allows
            at(70, 10, 2.0, W, H), at(70, 20, 2.0, W, H), at(80, 10, 2.0, W, H),
            at(32, 4, 2.0, W, H), at(32, 8, 2.0, W, H), at(32.2, 4, 4.0, W, H),
        ]
        f = [[0, 1, 2], [3, 4, 5], [6, 8, 7], [9, 11, 10], [12, 14, 13], [15, 17, 16], [18, 19, 19], [21, 22, 1000], [23, 24, 25], [26, 28, 27], [29, 30, 31]]
        image = noise_image(W, H, 50 + C)
        views = [_view(image, depth="mesh", min_cos=0.3), _view(image, depth=None, min_cos=0.3), _view(image, depth="mesh", min_cos=0.3, two_sided=True)]
        return _case(v, f, views, cell=C, colours=mr._rainbow(len(v), 31))
    return make


def _edges():
    """Projections on the image's edge: a face whose corners sit exactly on the centres of the first and the last pixels (its gutter falls off the image while
    its interior is inside), and a camera block of another size."""
    W, H = 16, 16
    v = [at(0.5, 0.5, 1.0, W, H), at(0.5, H - 0.5, 1.0, W, H), at(W - 0.5, 0.5, 1.0, W, H), at(W - 0.5, H - 0.5, 1.0, W, H)]
    f = [[0, 2, 1], [3, 1, 2]]
    views = [_view(noise_image(W, H, 60)), _view(noise_image(W, H, 61), camera=crafted_camera(W, H, block_size=(8, 8))), _view(ramp_image(W, H))]
    return _case(v, f, views, cell=8)


def _resolve_rules(colours, min_weight):
    """Faces of which a view colours some texels only -- a narrow photograph-sized window onto large charts -- so that the resolve meets baked texels, texels
    to fill from one, three and more neighbours, and texels with none."""
    def make():
        W, H = 8, 6
        # each face is far larger than the image: a few texels of its chart project inside
        v = [at(-4, -4, 4.0, W, H), at(-4, 10, 4.0, W, H), at(12, -4, 4.0, W, H), at(12, 10, 4.0, W, H),
             at(3, 2, 1.0, W, H), at(3, 3.2, 1.0, W, H), at(4.2, 2, 1.0, W, H)]
        f = [[0, 2, 1], [3, 1, 2], [4, 6, 5]]
        views = [_view(noise_image(W, H, 70), min_cos=0.2), _view(noise_image(W, H, 71), min_cos=0.9)]
        return _case(v, f, views, cell=16, colours=mr._rainbow(len(v), 41) if colours else None, min_weight=min_weight, fill=True)
    return make


def _three_views():
    W, H = 48, 40
    v, f = _tiles(40, W, H, 77, jitter=0.3)
    views = [_view(noise_image(W, H, 80 + k), depth="mesh" if k != 1 else None, min_cos=0.1 * k) for k in range(3)]
    return _case(v, f, views, cell=8, colours=mr._rainbow(v.shape[0], 42))


FACE_COUNTS = (0, 1, 2, 3, 7, 11, 129)


def _count_cases():
    out = {}
    for a, F in enumerate(FACE_COUNTS):
        for b, C in enumerate(CELLS):
            out[f"faces-{F}-cell-{C}"] = _counts(F, C, 4 * a + b)
    out["faces-18-cell-4"] = _counts(18, 4, 90)   # nine cells of 16 texels: two waves and a quarter, the wave's tail
    return out


CASES = dict({f"geometry-cell-{C}": _geometry(C) for C in CELLS},
             **{"edges": _edges, "resolve-colours": _resolve_rules(True, 1), "resolve-no-colours": _resolve_rules(False, 1), "resolve-min-weight-300": _resolve_rules(True, 300),
                "resolve-min-weight-600": _resolve_rules(True, 600), "three-views": _three_views}, **_count_cases())
THREE_VIEWS = "three-views"
# what the definition gives, where the case is about it: the face totals over the three views.  Per view: faces 0, 1, 7 and 8 are invalid; 9 is off the
# image; 3 faces away unless two-sided; 6 (zero area) and 10 (grazing) have Q = 0 at every corner
EXPECT = {f"geometry-cell-{C}": dict(invalidFaces=12, facingAwayFaces=3 + 3 + 2, offImageFaces=3, viewportMismatch=0) for C in CELLS}
EXPECT["edges"] = dict(invalidFaces=0, facingAwayFaces=0, offImageFaces=0, viewportMismatch=1)


def mesh_depth(m, w):
    """The depth image of case ``m``'s mesh under view ``w``, as ``MeshRasterizer.encode`` writes it."""
    return mr.rasterize(m["vertices"], m["faces"], None, w["camera"], w["width"], w["height"], w["near"], "none")["depth"]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, its ``"mesh"`` depths rasterized; computed once and shared: callers leave it unchanged."""
    m = CASES[name]()
    for w in m["views"]:
        if isinstance(w["depth"], str):
            w["depth"] = np.ascontiguousarray(mesh_depth(m, w), F32).reshape(w["height"], w["width"])
    for a in [m["vertices"], m["faces"], m["colours"]] + [x for w in m["views"] for x in w.values()]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def run(m, order=None):
    """``dict(rows, texture, texelState, totals)``: the views of case ``m`` accumulated in ``order`` (default: as listed) and resolved."""
    F = m["faces"].shape[0]
    state = new_state(F, m["cell"])
    for k in (range(len(m["views"])) if order is None else order):
        w = m["views"][k]
        accumulate(state, m["vertices"], m["faces"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"],
                   w["two_sided"])
    texture, tstate = resolve(state, m["faces"], m["colours"], m["vertices"].shape[0], m["min_weight"], m["fill"])
    return dict(rows=state["rows"].astype(np.uint32), texture=texture, texelState=tstate, totals=state["totals"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """``run`` of that case; computed once and shared: callers leave it unchanged."""
    out = run(case(name))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def digest(result):
    """sha256 over rows, texture, texel states and the totals (what a host's run script prints)."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(result["rows"], np.uint32).tobytes())
    h.update(np.ascontiguousarray(result["texture"], np.uint8).tobytes())
    h.update(np.ascontiguousarray(result["texelState"], np.uint8).tobytes())
    h.update(np.array([result["totals"][k] for k in STATS], np.uint64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- the analytic check: a fronto-parallel quad under a linear ramp
def analytic_scene(C, W=64, H=48):
    """A two-face quad parallel to the image plane and a photograph that is a linear ramp of at most one level a pixel on each axis: ``dict`` of the case
    and ``ramp(sx, sy)``, the ramp at a position in pixel coordinates (pixel centres at half-integers), per channel."""
    v, f = _quad(W, H, z=2.0, x0=5.3, y0=4.6, x1=W - 6.1, y1=H - 5.2)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = np.stack([np.rint(10 + 1.0 * i + 0.75 * j), np.rint(200 - 0.5 * i - 1.0 * j), np.rint(30 + 0.25 * i + 0.5 * j), np.full(i.shape, 255)], axis=2).astype(np.uint8)
    def ramp(sx, sy):
        i, j = np.asarray(sx, np.float64) - 0.5, np.asarray(sy, np.float64) - 0.5
        return np.stack([10 + 1.0 * i + 0.75 * j, 200 - 0.5 * i - 1.0 * j, 30 + 0.25 * i + 0.5 * j], axis=-1)
    return dict(case=_case(v, f, [_view(image, min_cos=0.1)], cell=C), ramp=ramp)


def analytic_errors(scene, texture, tstate):
    """Per baked interior texel (inside its face's triangle: i' + j' <= m) of the scene's atlas: ``|texture - ramp at the texel's own projection|``, the
    projection computed in doubles from the mesh, not by the definition's steps.  ``(errors f64[n, 3], n)``."""
    m = scene["case"]
    C, F = m["cell"], m["faces"].shape[0]
    W, H = m["views"][0]["width"], m["views"][0]["height"]
    tx = texels(F, C)
    inside = tx["ip"] + tx["jp"] <= C - 3
    baked = np.asarray(tstate)[tx["y"], tx["x"]] == 1
    sel = inside & baked
    corners = m["vertices"].astype(np.float64)[m["faces"].astype(np.int64)[tx["face"][sel]]]   # [n, 3, 3]; the crafted view is the identity
    u, v = tx["ip"][sel] / (C - 3.0), tx["jp"][sel] / (C - 3.0)
    p = (1 - u - v)[:, None] * corners[:, 0] + u[:, None] * corners[:, 1] + v[:, None] * corners[:, 2]
    sx, sy = (p[:, 0] / p[:, 2] * 0.5 + 0.5) * W, (-p[:, 1] / p[:, 2] * 0.5 + 0.5) * H
    got = np.asarray(texture)[tx["y"][sel], tx["x"][sel], :3].astype(np.float64)
    return np.abs(got - scene["ramp"](sx, sy)), int(sel.sum())


# ---------------------------------------------------------------- the icosphere under the zoo's cameras
SPHERE_CAMERAS = ("roll37", "below", "close")


@functools.lru_cache(maxsize=None)
def sphere(camera_name):
    """``meshraster_ref``'s icosphere case under that camera, with a noise photograph and its own depth image."""
    m = mr.case(f"sphere-{camera_name}")
    image = noise_image(m["width"], m["height"], 140 + SPHERE_CAMERAS.index(camera_name))
    depth = np.ascontiguousarray(mr.expected(f"sphere-{camera_name}")["depth"], F32).reshape(m["height"], m["width"])
    for a in (image, depth):
        a.setflags(write=False)
    return dict(m, image=image, depth=depth)
