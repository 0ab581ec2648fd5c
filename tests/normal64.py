"""Float64 restatement of the normal maps' definition, for the normal tests.

Per Gaussian (``gaussian_normals64``), from the record's fp16 fields: ``k`` the index of the smallest log-scale (ties: the lowest index), the world
normal row ``k`` of ``R(q / |q|)`` (``R`` as csrc/wgslm.h builds it: the rows of the matrix whose columns ``M3`` is given), the view-space normal the
upper 3x3 of the camera's view matrix times it, renormalised, negated where ``n . p > 0`` (``p`` the view-space centre).  No normal: ``|q| = 0`` or
a non-finite half among position, quaternion and log-scales.  The packed word (``encode64`` / ``decode64``): octahedral, snorm16 x 2, the ``z > 0``
hemisphere folded.  Compositing (``composite64``) is tests/depth64.py's walk, taken once per component with the normal's component in the place of the
depth: the same active records, the same float64 weights, the same ``near_saturation`` mask.  ``depth_normals64``, ``agreement64`` and
``normal_to_rgba8_64`` restate the three image kernels."""
import numpy as np

import depth64 as d64

NO_NORMAL = 0x80008000
SNORM = 32767.0
U = 2.0 ** -24            # unit roundoff of binary32
NEAR_FLIP = 1e-4          # |n^ . p^| below this: the f32 evaluation of the dot (error a few 1e-7) may fall on the other side of 0

# ---- bounds, derived (u = 2^-24; every f32 operation rounds once, relative error <= u)
# The unit view-space normal in f32 against float64, per component and in Euclidean norm: q / |q| is 4 products, 3 sums, a root and a quotient
# (<= 5u relative); an entry of R is at most 6 operations on values <= 1 in size and at most 2 in result (<= 8u absolute, with the 5u of q twice over
# in each product: <= 8u + 2 * 2 * 5u = 28u); the view transform (entries <= 1: a rotation) is 3 products and 2 sums of them (<= 3 * 28u + 5u = 89u
# over the three terms, the triangle inequality at its worst); the renormalisation 5u more.  F32_NORMAL = 96u covers it.
F32_NORMAL = 96 * U
# The octahedral coordinates o = n.xy / s, s = |n|_1 in [1, sqrt 3]: |do| <= |dn| / s + |n| |ds| / s^2 <= F + 3F, and 4 roundings of their own; the
# fold is 1-Lipschitz.  Rounding to the snorm16 grid adds half a step.  Decoding is the map (x, y) -> p = (x, y, 1 - |x| - |y|) -> p / |p|: |dp| <=
# sqrt(1 + 1 + 4) |d(x, y)|_inf, |p| >= 1 / sqrt 3, and x -> x / |x| is 1 / |p|-Lipschitz outside that ball: a factor sqrt 18.  The decode's own f32
# operations (2 quotients, 2 differences, 3 products, 2 sums, a root, 3 quotients): 12u.
QUANT_STEP = 0.5 / SNORM
ROUND_TRIP = np.sqrt(18.0) * QUANT_STEP * (1 + 1e-9)                                   # float64 encode + float64 decode of a unit vector
WORD_BOUND = np.sqrt(18.0) * (QUANT_STEP + 4 * F32_NORMAL + 4 * U) + 12 * U            # the GPU's word, decoded in f32, against the float64 normal


def halves(gaussians_u32):
    """The records' twelve halves as float64 ``[N, 12]``: x y z opacity | q (r, x, y, z) | log-scales x y z, pad (``project.hip: project_one``)."""
    return np.ascontiguousarray(gaussians_u32, np.uint32).reshape(-1, 6).view(np.float16).reshape(-1, 12).astype(np.float64)


def quat_to_rows(q):
    """``R`` of a quaternion ``[N, 4]`` (r, x, y, z) as ``[N, 3, 3]`` with ``out[:, r, c]`` = element r of column c of csrc/wgslm.h's ``quat_to_R``
    (``M3``'s arguments are columns): ``out[:, k, :]`` is row k."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    c0 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], axis=1)
    c1 = np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], axis=1)
    c2 = np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1)
    return np.stack([c0, c1, c2], axis=2)


def covariance64(q, scale):
    """``covariance3D(q, s) = M^T M``, ``M = diag(s) R`` (csrc/wgslm.h), ``[N, 3, 3]`` float64, for the quaternion as given (not normalised)."""
    R = quat_to_rows(q)
    M = scale[:, :, None] * R
    return np.einsum("nki,nkj->nij", M, M)


def gaussian_normals64(gaussians_u32, camera):
    """dict: ``normal`` ``[N, 3]`` (zero where there is none), ``valid`` ``[N]``, ``k`` ``[N]``, ``facing`` = ``n^ . p^`` before the flip (what ``near_flip``
    is taken from), ``unflipped`` the view-space normal before the flip, ``world`` the world normal, ``tie`` (the smallest log-scale occurs twice)."""
    h = halves(gaussians_u32)
    n = h.shape[0]
    pos, q, ls = h[:, 0:3], h[:, 4:8], h[:, 8:11]
    with np.errstate(invalid="ignore"):
        qq = np.sum(q * q, axis=1)
    valid = np.isfinite(pos).all(axis=1) & np.isfinite(q).all(axis=1) & np.isfinite(ls).all(axis=1)
    valid &= np.where(valid, qq, 0.0) > 0
    k = np.zeros(n, np.int64)
    sk = ls[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for i in (1, 2):
            less = ls[:, i] < sk
            k = np.where(less, i, k)
            sk = np.where(less, ls[:, i], sk)
        tie = (ls == sk[:, None]).sum(axis=1) > 1
    qs = np.where(valid[:, None], q, np.array([1.0, 0, 0, 0]))
    qh = qs / np.sqrt(np.sum(qs * qs, axis=1))[:, None]
    world = quat_to_rows(qh)[np.arange(n), k, :]
    cam = np.asarray(camera, np.float32).reshape(68).astype(np.float64)
    view = cam[0:16].reshape(4, 4).T          # row-major: view[r, c]
    nv = world @ view[:3, :3].T
    nv = nv / np.linalg.norm(nv, axis=1)[:, None]
    p = np.where(valid[:, None], pos, 0.0) @ view[:3, :3].T + view[:3, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        facing = np.sum(nv * p, axis=1) / np.linalg.norm(p, axis=1)
    flip = np.sum(nv * p, axis=1) > 0
    normal = np.where(flip[:, None], -nv, nv)
    normal[~valid] = 0
    return dict(normal=normal, valid=valid, k=k, facing=facing, unflipped=nv, world=world, tie=tie & valid)


def encode64(n):
    """The packed word of unit vectors ``[N, 3]`` (float64 arithmetic; the rounding is numpy's round-half-even, the GPU's ``rint``)."""
    n = np.asarray(n, np.float64)
    s = np.abs(n).sum(axis=1)
    ox, oy = n[:, 0] / s, n[:, 1] / s
    fold = n[:, 2] > 0
    fx = np.where(fold, np.copysign(1 - np.abs(oy), ox), ox)
    fy = np.where(fold, np.copysign(1 - np.abs(ox), oy), oy)
    qx = np.clip(np.rint(fx * SNORM), -SNORM, SNORM).astype(np.int64)
    qy = np.clip(np.rint(fy * SNORM), -SNORM, SNORM).astype(np.int64)
    return ((qx & 0xFFFF) | ((qy & 0xFFFF) << 16)).astype(np.uint32)


def decode64(words):
    """The decode of DESIGN.md section 12 in float64: unit vectors ``[N, 3]``, the zero vector for ``NO_NORMAL``."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    u = (w & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.float64) / SNORM
    v = (w >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(np.float64) / SNORM
    t = (1 - np.abs(u)) - np.abs(v)
    fold = t < 0
    x = np.where(fold, np.copysign(1 - np.abs(v), u), u)
    y = np.where(fold, np.copysign(1 - np.abs(u), v), v)
    out = np.stack([x, y, -t], axis=1)
    out = out / np.linalg.norm(out, axis=1)[:, None]
    out[w == np.uint32(NO_NORMAL)] = 0
    return out


def _ordered(x_f32):
    """The forward pass's order-preserving key of an f32 (``project.hip: ordered_uint``), which ``depth64.decode_depths`` inverts."""
    bits = np.ascontiguousarray(x_f32, np.float32).view(np.uint32)
    return bits ^ np.where(bits & np.uint32(0x80000000), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def composite64(settings, tinfo, stages, normals_f32, max_entries=0, tiles=None):
    """``A`` ``[H, W]``, ``N`` ``[H, W, 3]`` float64, ``near_saturation`` and ``n_active``: depth64's walk over the forward ``stages``
    (``HipPipeline.collect_forward`` / ``oracle.forward``), once per component, the per-Gaussian f32 normals ``[n, 3]`` standing where the depths stand.
    ``tiles`` (a boolean per tile, optional): only these tiles are walked -- the others are handed to the walk as empty and come back all zero."""
    normals_f32 = np.ascontiguousarray(normals_f32, np.float32)
    ranges = np.array(stages["tile_ranges"], np.uint32)
    if tiles is not None:
        ranges[:len(tiles)][~np.asarray(tiles, bool)] = 0xFFFFFFFF
    comps, A, near_sat, stats = [], None, None, {}
    for c in range(3):
        stats = {}
        A, D, _, near_sat, _ = d64.depth64(settings, tinfo, stages["splats"], _ordered(normals_f32[:, c]), ranges, stages["sorted_keys"],
                                           stages["sorted_values"], stages["total_entries"], max_entries=max_entries, stats=stats)
        comps.append(D * A)   # (depth64 hands out S / A: S again, to a relative 2^-52)
    return A, np.stack(comps, axis=2), near_sat, stats["n_active"]


def tile_pixels(tiles, width, height):
    """The ``[H, W]`` mask of the pixels of the tiles selected by ``tiles`` (a boolean per 16 x 16 tile, row-major)."""
    ntx, nty = (width + 15) // 16, (height + 15) // 16
    return np.kron(np.asarray(tiles, bool).reshape(nty, ntx), np.ones((16, 16), bool))[:height, :width]


def depth_normals64(depth, p00, p11):
    """The stencil of ``wdgs_depth_to_normals`` in float64 on an ``[H, W]`` depth image: ``normal`` ``[H, W, 3]`` (zero where invalid), ``valid``, and
    per pixel the quantities its f32 error bound is made of: ``cross`` = |a x b|, ``a`` = |a|, ``b`` = |b|, ``zmax`` the largest |coordinate| among the
    five points (all zero where invalid)."""
    d = np.asarray(depth, np.float64)
    H, W = d.shape
    p00, p11 = float(np.float32(p00)), float(np.float32(p11))
    jj, ii = np.mgrid[0:H, 0:W]
    ndc_x = 2.0 * (ii + 0.5) / W - 1.0
    ndc_y = 1.0 - 2.0 * (jj + 0.5) / H
    with np.errstate(invalid="ignore", over="ignore"):
        V = np.stack([ndc_x * d / p00, ndc_y * d / p11, d], axis=2)
    has = (d > 0) & np.isfinite(d)
    valid = np.zeros((H, W), bool)
    valid[1:-1, 1:-1] = has[1:-1, 1:-1] & has[1:-1, :-2] & has[1:-1, 2:] & has[:-2, 1:-1] & has[2:, 1:-1]
    a = np.zeros((H, W, 3)); b = np.zeros((H, W, 3)); zmax = np.zeros((H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        a[1:-1, 1:-1] = V[1:-1, 2:] - V[1:-1, :-2]
        b[1:-1, 1:-1] = V[2:, 1:-1] - V[:-2, 1:-1]
        zmax[1:-1, 1:-1] = np.max(np.abs(np.stack([V[1:-1, 1:-1], V[1:-1, 2:], V[1:-1, :-2], V[2:, 1:-1], V[:-2, 1:-1]])), axis=(0, 3))
        c = np.cross(a, b)
        length = np.linalg.norm(c, axis=2)
        valid &= np.isfinite(length) & (length > 0)
        n = np.where(valid[..., None], c / np.where(valid, length, 1.0)[..., None], 0.0)
        flip = np.sum(n * np.where(valid[..., None], V, 0.0), axis=2) > 0
    n = np.where(flip[..., None], -n, n)
    z = np.zeros((H, W))
    return dict(normal=n, valid=valid, cross=np.where(valid, length, z), a=np.where(valid, np.linalg.norm(a, axis=2), z),
                b=np.where(valid, np.linalg.norm(b, axis=2), z), zmax=np.where(valid, zmax, z))


def depth_normals_f32_bound(dn):
    """Per pixel, the f32 kernel's normal against ``depth_normals64`` of the same f32 depth image (Euclidean norm of the difference).  A point's
    coordinate is 5 operations (<= 5u relative, of size <= Z = ``zmax``); a difference of two, 11u Z absolute per component, sqrt(3) times that as a
    vector; the cross product is off by |da| |b| + |a| |db| plus its own three roundings per component (<= 3u |a| |b| sqrt 3); dividing by its length
    |c| turns that into the direction's error (x -> x / |x| is 1 / |c|-Lipschitz; a factor 2 for the second order), and the normalisation's own
    operations add 6u."""
    Z, a, b, c = dn["zmax"], dn["a"], dn["b"], dn["cross"]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(dn["valid"], 2.0 * np.sqrt(3.0) * U * (11.0 * Z * (a + b) + 3.0 * a * b) / np.where(c > 0, c, 1.0) + 6.0 * U, 0.0)


def agreement64(comp_f32, dn_f32):
    """The sums of ``wdgs_normal_agreement`` from the two f32 images ``[H, W, 4]``: ``(sum_e, sum_a, pixels)`` with the per-pixel terms in float64
    (``sum_a`` is exact either way: ``A 2^24`` is an integer for an f32 ``A >= 0.5``).  The predicate ``|N| > 0`` is the kernel's, on its f32 sum of
    squares."""
    comp, dn = np.asarray(comp_f32, np.float32), np.asarray(dn_f32, np.float32)
    N, A = comp[..., :3], comp[..., 3]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        l2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        counted = (A >= 0.5) & np.isfinite(A) & (l2 > 0) & np.isfinite(l2) & (dn[..., 3] != 0)
    N64, A64 = N[counted].astype(np.float64), A[counted].astype(np.float64)
    c = np.sum(N64 / np.linalg.norm(N64, axis=1)[:, None] * dn[..., :3][counted].astype(np.float64), axis=1)
    e = np.rint(A64 * np.maximum(1.0 - c, 0.0) * 2.0 ** 24)
    a = np.rint(A64 * 2.0 ** 24)
    return int(e.sum()), int(a.sum()), int(counted.sum())


# Per counted pixel, |e_gpu - e_64| in units of 2^-24.  The f32 cosine: the sum of squares, its root and the three quotients leave N / |N| within 3.5u
# relative per component; the three products with n_d and their two sums add 1u and 2u of sum |n_i d_i| <= 1 (two unit vectors): <= 7u, 12u taken.
# Times A 2^24 <= 2^24: 12 units.  1 - c and the product with A round once each: 2u relative of A (1 - c) 2^24 <= 2^25, 4 units.  The two rints: half
# a unit each.
AGREEMENT_UNITS_PER_PIXEL = 12 + 4 + 1


def normal_to_rgba8_64(img):
    """The presentation formula in float64 on an ``[H, W, 4]`` normal image: rgb ``[H, W, 3]`` uint8, and the float64 ``255 c`` they were rounded from
    (black, 0, where ``|N|`` is not > 0)."""
    N = np.asarray(img, np.float32)[..., :3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2])
        ok = (length > 0) & np.isfinite(length)
        n = N / np.where(ok, length, 1.0)[..., None]
    v = 255.0 * (0.5 + 0.5 * n * np.array([1.0, -1.0, -1.0]))
    v = np.where(ok[..., None], v, 0.0)
    return np.floor(v + 0.5).astype(np.uint8), v
