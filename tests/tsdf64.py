"""Float64 restatement of TSDF fusion and of marching tetrahedra, for the TSDF tests.

``integrate64`` fuses one view into a ``Volume64``.  Every quantity is formed twice from the same float32 inputs (origin, voxel size, camera block,
depth): in float32, operation by operation in the library's order (``f32`` below; numpy's float32 arithmetic is IEEE and unfused, as the library's
under ``-ffp-contract=off``), and in float64.  The DECISIONS -- ``z > 0``, the pixel, ``sdf < -truncation`` -- are taken twice as well: set ``A`` on
the float32 values, as the library takes them, and set ``B`` on the float64 values.  Given a decision, the observation ``t = min(sdf / truncation, 1)``
and the running mean are float64 (``sdf`` the float64 one).  Where the float64 value lies within ``EPS`` of a decision's boundary the voxel is masked
for that view: ``near_edge`` (``px`` within ``EPS_PIXEL W`` or ``py`` within ``EPS_PIXEL H`` of an integer, the image borders among them -- the
error of either is that of a ratio of size <= 1, scaled by the image's size), ``near_cut`` (``sdf`` within
``EPS_SDF * truncation`` of ``-truncation``) and ``near_zero_z`` (``|z| < EPS_Z``).  Outside the masks A and B decide alike
(tests/test_tsdf_reference.py asserts it), so there the library has one right answer.

``mesh64`` restates marching tetrahedra on the Kuhn split.  Its cases are not the kernel's table: for every tetrahedron and sign pattern the
triangles' vertex ORDER comes from the rule of DESIGN.md section 13 (which edge is first) and their WINDING from geometry -- the normal of the
triangle through the edge midpoints must point from the inside corners' centroid to the outside corners'.
"""
import itertools

import numpy as np

# 8 x the largest |f32 - f64| observed on the test scenes (the sphere scene and the 96^3 volume of the 20 000-point scene; DESIGN.md section 13 has the
# observed values): px / W and py / H, sdf in units of the truncation, z in world units.
EPS_PIXEL = 2.5e-6
EPS_SDF = 4e-5
EPS_Z = 1e-4
U = 2.0 ** -24   # half an ulp of 1: the relative error of one float32 rounding

# roundings between the float32 inputs and sdf / truncation, each counted at the scale of the largest intermediate (|coordinate| + depth): the voxel
# centre (2 per axis), three products and three sums of the view row, d - z, and the quotient
SDF_ROUNDINGS = 14


class Volume64:
    """The volume's state in float64 (weights are small integers, exact in either format), arrays ``[nz, ny, nx]``, colour ``[3, nz, ny, nx]``."""

    def __init__(self, origin, voxel_size, dims, truncation, max_weight=64.0, colour=True):
        self.origin = np.asarray(origin, np.float32).reshape(3)
        self.voxel_size = np.float32(voxel_size)
        self.dims = tuple(int(d) for d in dims)
        self.truncation = np.float32(truncation)
        self.max_weight = float(max_weight)
        nx, ny, nz = self.dims
        self.T = np.ones((nz, ny, nx))
        self.W = np.zeros((nz, ny, nx))
        self.rgb = np.zeros((3, nz, ny, nx)) if colour else None
        self.views = 0

    def copy(self):
        c = Volume64(self.origin, self.voxel_size, self.dims, self.truncation, self.max_weight, self.rgb is not None)
        c.T, c.W, c.views = self.T.copy(), self.W.copy(), self.views
        c.rgb = None if self.rgb is None else self.rgb.copy()
        return c

    def centres32(self):
        """The voxel centres per axis as the library forms them: origin + ((float)i + 0.5) voxel_size, in float32."""
        return [self.origin[a] + (np.arange(self.dims[a], dtype=np.float32) + np.float32(0.5)) * self.voxel_size for a in range(3)]

    def centres64(self):
        return [float(self.origin[a]) + (np.arange(self.dims[a], dtype=np.float64) + 0.5) * float(self.voxel_size) for a in range(3)]


def _grid(cs):
    """x, y, z coordinate arrays [nz, ny, nx] from the per-axis centres."""
    cz, cy, cx = np.meshgrid(cs[2], cs[1], cs[0], indexing="ij")
    return cx, cy, cz


def project(vol, camera, width, height):
    """Per voxel, in float32 as the library and in float64: ``dict(z32, px32, py32, z64, px64, py64, scale)``; ``scale`` is the largest
    |intermediate| of the view row (the sum of the |terms|)."""
    blk = np.asarray(camera, np.float32).reshape(68)
    f = np.float32
    x, y, z = _grid(vol.centres32())
    row = lambda r: ((blk[0 + r] * x + blk[4 + r] * y) + blk[8 + r] * z) + blk[12 + r]   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vx, vy, vz = row(0), row(1), row(2)
        px = (((blk[32] * vx) / vz) * f(0.5) + f(0.5)) * f(width)
        py = ((((-blk[37]) * vy) / vz) * f(0.5) + f(0.5)) * f(height)
    assert px.dtype == np.float32 and vz.dtype == np.float32
    b = blk.astype(np.float64)
    X, Y, Z = _grid(vol.centres64())
    row64 = lambda r: b[0 + r] * X + b[4 + r] * Y + b[8 + r] * Z + b[12 + r]   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        VX, VY, VZ = row64(0), row64(1), row64(2)
        PX = ((b[32] * VX) / VZ * 0.5 + 0.5) * width
        PY = (((-b[37]) * VY) / VZ * 0.5 + 0.5) * height
    scale = float((np.abs(b[2] * X) + np.abs(b[6] * Y) + np.abs(b[10] * Z) + abs(b[14])).max())
    return dict(z32=vz, px32=px, py32=py, z64=VZ, px64=PX, py64=PY, scale=scale)


def _decide(z, px, py, depth, weight_sum, min_weight_sum, width, height, truncation, sdf_of):
    """The library's chain of skips on one set of values: (updated, pixel index, sdf, what reaches the sdf test)."""
    with np.errstate(invalid="ignore"):
        ok = (z > 0) & (px >= 0) & (px < width) & (py >= 0) & (py < height)
    ix = np.where(ok, px, 0).astype(np.int64)
    iy = np.where(ok, py, 0).astype(np.int64)
    p = iy * int(width) + ix
    d = depth[p]
    with np.errstate(invalid="ignore"):
        ok &= (d > 0) & (d < np.inf)
        if weight_sum is not None:
            ok &= weight_sum[p] >= np.float32(min_weight_sum)
        sdf = sdf_of(d)
        pre = ok.copy()
        ok &= ~(sdf < -truncation)
    return ok, p, sdf, pre


def integrate64(vol_a, vol_b, depth, camera, width, height, weight_sum=None, colour=None, min_weight_sum=0.5):
    """Fuses one view into ``vol_a`` (decisions on the float32 values, as the library takes them) and ``vol_b`` (decisions on the float64 values; may be
    None).  Returns ``dict(near_edge, near_cut, near_zero_z, updated_a, updated_b, scale, max_depth, dist_px, dist_sdf)``: the masks ``[nz, ny, nx]``,
    and the largest |f32 - f64| of px / W, py / H and of sdf / truncation over the voxels both sets update."""
    depth = np.asarray(depth, np.float32).reshape(-1)
    assert depth.size == width * height
    ws = None if weight_sum is None else np.asarray(weight_sum, np.float32).reshape(-1)
    col = None if colour is None else np.asarray(colour, np.uint8).reshape(-1, 4)
    pr = project(vol_a, camera, width, height)
    trunc32, trunc = vol_a.truncation, float(vol_a.truncation)

    ok_a, p_a, sdf32, _ = _decide(pr["z32"], pr["px32"], pr["py32"], depth, ws, min_weight_sum, np.float32(width), np.float32(height), trunc32, lambda d: d - pr["z32"])
    ok_b, p_b, sdf64_b, pre_b = _decide(pr["z64"], pr["px64"], pr["py64"], depth, ws, min_weight_sum, float(width), float(height), trunc,
                                 lambda d: d.astype(np.float64) - pr["z64"])

    def update(vol, ok, p):
        sdf = depth[p].astype(np.float64) - pr["z64"]
        t = np.minimum(sdf / trunc, 1.0)
        q = vol.W + 1.0
        vol.T = np.where(ok, (vol.T * vol.W + t) / q, vol.T)
        if col is not None and vol.rgb is not None:
            for c in range(3):
                vol.rgb[c] = np.where(ok, (vol.rgb[c] * vol.W + col[p, c] / 255.0) / q, vol.rgb[c])
        vol.W = np.where(ok, np.minimum(q, vol.max_weight), vol.W)
        vol.views += 1

    update(vol_a, ok_a, p_a)
    if vol_b is not None:
        update(vol_b, ok_b, p_b)

    # the masks, on the float64 values
    with np.errstate(invalid="ignore"):
        z64, px64, py64 = pr["z64"], pr["px64"], pr["py64"]
        near_zero_z = np.abs(z64) < EPS_Z
        front = z64 > 0
        frac = lambda v: np.abs(v - np.rint(v))   # noqa: E731
        ex, ey = EPS_PIXEL * width, EPS_PIXEL * height
        band = (px64 > -ex) & (px64 < width + ex) & (py64 > -ey) & (py64 < height + ey)
        near_edge = front & band & ((frac(px64) < ex) | (frac(py64) < ey))
        near_cut = pre_b & (np.abs(sdf64_b + trunc) < EPS_SDF * trunc)
        both = ok_a & ok_b
        dist_px = float(max(np.abs(pr["px32"].astype(np.float64) - px64)[both].max(initial=0.0) / width,
                            np.abs(pr["py32"].astype(np.float64) - py64)[both].max(initial=0.0) / height))
        dist_sdf = float((np.abs(sdf32.astype(np.float64) - sdf64_b)[both & (p_a == p_b)] / trunc).max(initial=0.0))
    return dict(near_edge=near_edge, near_cut=near_cut, near_zero_z=near_zero_z, updated_a=ok_a, updated_b=ok_b, scale=pr["scale"],
                max_depth=float(depth[np.isfinite(depth)].max(initial=0.0)), dist_px=dist_px, dist_sdf=dist_sdf)


def tsdf_bound(scale, max_depth, truncation, views):
    """|T - T64| outside the masks: SDF_ROUNDINGS roundings at 2^-23 (|coordinate| + depth) / truncation, plus 2^-23 per fused view.  (Each rounding is
    half of that, so the first term has SDF_ROUNDINGS 2^-24 (...) to spare; the running mean's three roundings per view -- T Wt, the sum, the
    quotient: below 1.5 2^-23 together in units of T -- fit in the second term and that spare while views <= SDF_ROUNDINGS (...) / truncation.)"""
    s = (scale + max_depth) / float(truncation)
    assert views <= SDF_ROUNDINGS * s
    return SDF_ROUNDINGS * 2.0 ** -23 * s + views * 2.0 ** -23


# ---------------------------------------------------------------- marching tetrahedra
AXIS_PERMUTATIONS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]   # xyz, xzy, yxz, yzx, zxy, zyx


def tet_corners(t):
    """The four cell corners (0..7, bit a set = offset 1 along axis a) of tetrahedron t: 0, e_a, e_a + e_b, (1,1,1)."""
    a, b, _ = AXIS_PERMUTATIONS[t]
    return [0, 1 << a, (1 << a) | (1 << b), 7]


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64)


def tet_triangles(t, inside):
    """The triangles of tetrahedron t for the 4-tuple of booleans ``inside`` (per tetrahedron corner p0..p3): a list of triangles, each three edges
    (u, v) of CELL corners.  Order by the rule, winding by geometry (module docstring)."""
    corners = tet_corners(t)
    ins = [v for v in range(4) if inside[v]]
    outs = [v for v in range(4) if not inside[v]]
    if len(ins) in (0, 4):
        return []
    pos = [_corner_xyz(c) for c in corners]
    outward = np.mean([pos[v] for v in outs], axis=0) - np.mean([pos[v] for v in ins], axis=0)
    mid = lambda e: 0.5 * (pos[e[0]] + pos[e[1]])   # noqa: E731

    def wound(tri):
        n = np.cross(mid(tri[1]) - mid(tri[0]), mid(tri[2]) - mid(tri[0]))
        s = float(n @ outward)
        assert abs(s) > 1e-9
        return tri if s > 0 else [tri[0], tri[2], tri[1]]

    if len(ins) in (1, 3):
        lone = ins[0] if len(ins) == 1 else outs[0]
        rest = outs if len(ins) == 1 else ins
        tris = [wound([(lone, rest[0]), (lone, rest[1]), (lone, rest[2])])]
    else:
        (a, b), (c, d) = ins, outs
        q = [(a, c), (a, d), (b, d), (b, c)]
        tris = [wound([q[0], q[1], q[2]]), wound([q[0], q[2], q[3]])]
    return [[(corners[u], corners[v]) for u, v in tri] for tri in tris]


def mesh64(tsdf, weight, origin, voxel_size, min_weight=1.0, rgb=None):
    """Marching tetrahedra over a volume given as float32 arrays ``[nz, ny, nx]``: ``dict(keys u64[F,3], positions f64[F,3,3], colours f64[F,3,3] |
    None)``, cells in linear order, then tetrahedra, then triangles.  Positions (and colours, in [0, 1] units before rounding) are float64 from the
    float32 inputs."""
    T = np.asarray(tsdf, np.float32)
    Wt = np.asarray(weight, np.float32)
    nz, ny, nx = T.shape
    o = np.asarray(origin, np.float32).astype(np.float64)
    vs = float(np.float32(voxel_size))
    corner = lambda a, c: a[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]   # noqa: E731
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    inside = []
    for c in range(8):
        with np.errstate(invalid="ignore"):
            valid &= corner(Wt, c) >= np.float32(min_weight)
            inside.append(corner(T, c) < 0)
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell_lin = ((kk * (ny - 1) + jj) * (nx - 1) + ii)
    recs = []   # (cell, t, f, [3 x (linA, d)]) blocks
    for t in range(6):
        corners = tet_corners(t)
        for pattern in itertools.product([False, True], repeat=4):
            tris = tet_triangles(t, pattern)
            if not tris:
                continue
            sel = valid.copy()
            for v in range(4):
                sel &= inside[corners[v]] == pattern[v]
            if not sel.any():
                continue
            ci, cj, ck, cl = ii[sel], jj[sel], kk[sel], cell_lin[sel]
            for f, tri in enumerate(tris):
                ka = np.empty((cl.size, 3), np.int64)
                kd = np.empty((cl.size, 3), np.int64)
                for s, (u, v) in enumerate(tri):
                    a, b = min(u, v), max(u, v)
                    assert a & b == a   # Kuhn edges join nested offsets: the smaller is the corner of lower linear index
                    ka[:, s] = ((ck + ((a >> 2) & 1)) * ny + (cj + ((a >> 1) & 1))) * nx + (ci + (a & 1))
                    kd[:, s] = a ^ b
                recs.append((cl, np.full(cl.size, t), np.full(cl.size, f), ka, kd))
    if not recs:
        return dict(keys=np.zeros((0, 3), np.uint64), positions=np.zeros((0, 3, 3)), colours=None if rgb is None else np.zeros((0, 3, 3)))
    cl = np.concatenate([r[0] for r in recs]); tt = np.concatenate([r[1] for r in recs]); ff = np.concatenate([r[2] for r in recs])
    ka = np.concatenate([r[3] for r in recs]); kd = np.concatenate([r[4] for r in recs])
    order = np.lexsort((ff, tt, cl))
    ka, kd = ka[order], kd[order]
    keys = (ka.astype(np.uint64) * np.uint64(8) + (kd - 1).astype(np.uint64))
    Tf = T.reshape(-1).astype(np.float64)
    step = np.stack([kd & 1, (kd >> 1) & 1, (kd >> 2) & 1], axis=-1)
    kb = ka + step[..., 0] + step[..., 1] * nx + step[..., 2] * nx * ny
    w = Tf[ka] / (Tf[ka] - Tf[kb])
    idx = np.stack([ka % nx, (ka // nx) % ny, ka // (nx * ny)], axis=-1)
    pa = o + (idx + 0.5) * vs
    positions = pa + (step * vs) * w[..., None]
    colours = None
    if rgb is not None:
        C = np.asarray(rgb, np.float32).reshape(3, -1).astype(np.float64)
        colours = np.stack([C[c][ka] + (C[c][kb] - C[c][ka]) * w for c in range(3)], axis=-1)
    return dict(keys=keys, positions=positions, colours=colours)


def weld(keys, positions):
    """(vertices [V,3], faces [F,3]) by the distinct keys in ascending order."""
    uniq, first, inverse = np.unique(np.asarray(keys).reshape(-1), return_index=True, return_inverse=True)
    return np.asarray(positions).reshape(-1, 3)[first], inverse.reshape(-1, 3)


def mesh_topology(faces):
    """``dict(V, E, F, closed, consistent)``: ``closed`` when every undirected edge is in exactly two triangles, ``consistent`` when every directed edge
    occurs exactly once (so the two triangles of an edge run through it in opposite directions)."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    nv = int(faces.max()) + 1 if faces.size else 0
    directed = d[:, 0] * nv + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * nv + np.maximum(d[:, 0], d[:, 1])
    _, dc = np.unique(directed, return_counts=True)
    ue, uc = np.unique(und, return_counts=True)
    return dict(V=int(np.unique(faces).size), E=int(ue.size), F=int(faces.shape[0]), closed=bool(np.all(uc == 2)), consistent=bool(np.all(dc == 1)))
