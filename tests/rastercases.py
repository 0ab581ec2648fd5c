"""Crafted tile lists for the two raster kernels -- rasterize (K14, webdgs_amd/csrc/raster.hip) and backward_rasterize (K16,
backward_raster.hip) -- and a float64 restatement of what they compute.  Plain numpy: nothing here needs a GPU, the library or the oracle.

A case is a dict: a Splat table (u32[N, 6], the word layout project.hip writes: ndc x|y, extent x|y, conic x|y, conic z|0, r|g, b|opacity, all
fp16), the sorted (key, value) streams with key = (tile + 1) << 16 | depth16, the range table by lower-bound search, the viewport, the
settings the forward pass would carry (render mode, radius cap, point size, compat cap), and an rgba8 image pair with a lambda_l2 whose
difference is the loss gradient K16 is handed (lambda_l1 = lambda_dssim = 0: g = lambda_l2 (pred - targ) / 255 per pixel and channel).

THE DOMAIN (what project.hip can write and oracle_forward.cpp reads; the cases sit at its corners, not outside it):
  * every half is finite (non-finite Splats: tests/test_gpu_nan.py);
  * ndc centre in [-1.2, 1.2] (project.hip culls beyond), so a centre lies at most a tenth of the viewport outside the image;
  * extents >= 0 (a square root), stored BEFORE the kernels apply min(extent, cap) again;
  * conic: fp16 roundings of a positive definite matrix's entries -- x > 0, z > 0 before rounding, so a rounded x or z may be as small as the
    smallest subnormal half, and y may round past sqrt(x z): the quadratic form is then indefinite and the exponent's argument positive at
    some pixels; the covariance is dilated by 0.3 px^2, so x, z <= 1 / 0.3;
  * colour in [0, 1]; opacity in (1/128, 1] (project.hip culls 2 ln(128 o) <= 0);
  * values < num_splats -- except the explicit sentinel cases (family 1), whose values K14 must skip without counting them, as the
    reference does (tiled-rasterizer.wgsl:150, 197-201).  K16 is not told num_splats (nor is the reference's, which indexes the table with
    whatever the list holds): in those cases every value is a row of the table, and num_splats -- smaller than the table -- is K14's alone.

The float64 restatement follows the textbook forms, as indep64.py does: front-to-back compositing with the extent test, the 0.99 clamp and
stop and the 1/255 rule for n_contrib; the backward from suffix products and suffix sums (dC/dalpha_k = T_k c_k - sum_{j>k} c_j alpha_j T_j
/ (1 - alpha_k)), not from the kernels' running recurrences.  Where a viewport is a power of two, the pixel-space centre of an fp16 ndc value
is exact in float32 and float64 alike, and a case may put |d| exactly on an extent.
"""
import numpy as np

import sortcases as sc

EMPTY = sc.EMPTY
MIN_ALPHA = 1.0 / 255.0
STOP = 0.99
FIXED = 1.0e6
FLAT = 2.0 ** -24          # the smallest positive half: the widest conic a Splat can hold
NARROW = 1.0 / 0.3         # the narrowest isotropic conic (the 0.3 px^2 dilation)
EXCUSE = 1e-4              # a decision within this relative distance of its threshold is not float64's to call


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def f16v(x):
    """x rounded to a half, as float64."""
    return f16(x).astype(np.float64)


def f16_step(x, steps):
    """The half `steps` representable values away from the half x (positive finite x)."""
    b = f16(x).view(np.uint16).astype(np.int64) + int(steps)
    return np.array(b, np.uint16).view(np.float16).astype(np.float64)


def pack_rows(ndc_x, ndc_y, ex, ey, ca, cb, cc, r, g, b, op):
    """Splat rows u32[N, 6] from per-row values (each rounded to fp16)."""
    cols = [np.atleast_1d(f16(v)).view(np.uint16).astype(np.uint32) for v in (ndc_x, ndc_y, ex, ey, ca, cb, cc, r, g, b, op)]
    n = max(c.size for c in cols)
    c = [np.broadcast_to(v, n) for v in cols]
    z = np.zeros(n, np.uint32)
    lo_hi = [(c[0], c[1]), (c[2], c[3]), (c[4], c[5]), (c[6], z), (c[7], c[8]), (c[9], c[10])]
    return np.ascontiguousarray(np.stack([lo | (hi << 16) for lo, hi in lo_hi], 1).astype(np.uint32))


def unpack_rows(rows):
    h = np.ascontiguousarray(rows, np.uint32).view(np.float16).reshape(-1, 12).astype(np.float64)
    return dict(ndc=h[:, 0:2], ext=h[:, 2:4], conic=h[:, [4, 5, 6]], rgb=h[:, 8:11], op=h[:, 11])


def key_stream(lists, total_tiles):
    """lists: {tile: [values in list order]} -> (keys, vals, ranges[T + 1]); depth16 = the position in the tile's list (clamped)."""
    keys, vals = [], []
    for t in sorted(lists):
        v = np.asarray(lists[t], np.int64)
        keys.append(((t + 1) << 16) | np.minimum(np.arange(v.size), 0xFFFF))
        vals.append(v)
    keys = np.concatenate(keys).astype(np.uint32) if keys else np.zeros(0, np.uint32)
    vals = np.concatenate(vals).astype(np.uint32) if vals else np.zeros(0, np.uint32)
    return keys, vals, sc.expected_ranges(keys, total_tiles)


def default_images(W, H):
    y, x = np.mgrid[0:H, 0:W]
    pred = np.stack([(x * 7 + y * 13 + c * 29) % 256 for c in range(3)] + [np.full((H, W), 255)], 2).astype(np.uint8)
    targ = np.stack([(x * 5 + y * 3 + c * 17 + 128) % 256 for c in range(3)] + [np.full((H, W), 255)], 2).astype(np.uint8)
    return np.ascontiguousarray(pred), np.ascontiguousarray(targ)


class Scene:
    """Builder: splats by pixel-space centre, tile lists by hand."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.ntx, self.nty = (W + 15) // 16, (H + 15) // 16
        self.T = self.ntx * self.nty
        self.exact = (W & (W - 1)) == 0 and (H & (H - 1)) == 0
        self.rows, self.lists = [], {}

    def splat(self, cx, cy, ex, ey, conic=(FLAT, 0.0, FLAT), rgb=None, op=0.5):
        i = len(self.rows)
        if rgb is None:
            rgb = (((i * 37) % 64 + 1) / 64.0, ((i * 11) % 32) / 32.0, ((i * 5) % 16 + 1) / 16.0)
        self.rows.append((2.0 * cx / self.W - 1.0, 1.0 - 2.0 * cy / self.H, ex, ey, conic[0], conic[1], conic[2], rgb[0], rgb[1], rgb[2], op))
        return i

    def add(self, tile, *values):
        self.lists.setdefault(tile, []).extend(values)

    def origin(self, tile):
        return 16.0 * (tile % self.ntx), 16.0 * (tile // self.ntx)

    def case(self, name, family, **kw):
        rows = pack_rows(*np.array(self.rows, np.float64).T) if self.rows else np.zeros((1, 6), np.uint32)
        keys, vals, ranges = key_stream(self.lists, self.T)
        pred, targ = default_images(self.W, self.H)
        c = dict(name=name, family=family, W=self.W, H=self.H, rows=rows, num_splats=rows.shape[0], keys=keys, vals=vals, ranges=ranges,
                 count=int(keys.size), max_batches=0, mode=1, cap=0.0, point=0.0, lam=1.0, pred=pred, targ=targ, f64_backward=True, k16=True, claims={})
        c.update(kw)
        for a in (c["rows"], c["keys"], c["vals"], c["ranges"], c["pred"], c["targ"]):
            a.setflags(write=False)
        return c


# ----------------------------------------------------------------------------- what the kernels are handed
def effective_cap(case):
    cap = case["cap"] if case["cap"] != 0.0 else 128.0       # (0 = the default, as the host configuration has it)
    return cap if cap > 0.0 else 1e9


def settings_array(case, backward=False):
    """The 7-float RenderSettings block; the backward pass's own block has gaussian_mode = 0 (tiled-backward-pass.ts:150-159)."""
    cap = case["cap"] if case["cap"] != 0.0 else 128.0
    return np.array([1.0, 0.0, case["W"], case["H"], case["point"] if case["point"] != 0.0 else 3.0, 0.0 if backward else float(case["mode"]), cap], np.float32)


def tile_info_array(case):
    tx, ty = (case["W"] + 15) // 16, (case["H"] + 15) // 16
    return np.array([tx, ty, tx * ty, 0], np.uint32)


def loss_gradient64(case, pred=None, targ=None):
    p = (case["pred"] if pred is None else pred)[:, :, :3].astype(np.float64) / 255.0
    t = (case["targ"] if targ is None else targ)[:, :, :3].astype(np.float64) / 255.0
    return float(np.float32(case["lam"])) * (p - t)


def _geometry(case):
    u = unpack_rows(case["rows"])
    W, H, cap = case["W"], case["H"], effective_cap(case)
    u["cx"], u["cy"] = (0.5 * u["ndc"][:, 0] + 0.5) * W, (-0.5 * u["ndc"][:, 1] + 0.5) * H
    u["ex"], u["ey"] = np.minimum(u["ext"][:, 0], cap), np.minimum(u["ext"][:, 1], cap)
    return u


def _tile_pixels(case, t):
    ntx = (case["W"] + 15) // 16
    x0, y0 = 16 * (t % ntx), 16 * (t // ntx)
    ys, xs = np.mgrid[y0:min(y0 + 16, case["H"]), x0:min(x0 + 16, case["W"])]
    return ys.reshape(-1), xs.reshape(-1)


def forward_list(case, t):
    """The Gaussians K14 composites for tile t, in order: the tile's entries from ranges[t] to the key change, under the compat cap; values
    >= num_splats dropped WITHOUT a count; the walk ends at the first batch of 256 entries without a valid one (tiled-rasterizer.wgsl:187-192)."""
    start = int(case["ranges"][t])
    if start == EMPTY or start >= case["count"]:
        return np.zeros(0, np.int64)
    keys, vals = case["keys"], case["vals"]
    end = start
    while end < case["count"] and (int(keys[end]) >> 16) == t + 1:
        end += 1
    if case["max_batches"]:
        end = min(end, start + 256 * case["max_batches"])
    out = []
    for b in range(start, end, 256):
        v = vals[b:min(b + 256, end)].astype(np.int64)
        v = v[v < case["num_splats"]]
        if v.size == 0:
            break
        out.append(v)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def _alpha(u, g, px, py):
    """For Gaussians g[E] and pixel centres [P]: dx, dy, inside, G, alpha as [P, E] float64 arrays."""
    dx, dy = px[:, None] - u["cx"][g][None, :], py[:, None] - u["cy"][g][None, :]
    inside = (np.abs(dx) <= u["ex"][g][None, :]) & (np.abs(dy) <= u["ey"][g][None, :])
    c = u["conic"][g]
    q = c[None, :, 0] * dx * dx + 2.0 * c[None, :, 1] * dx * dy + c[None, :, 2] * dy * dy
    with np.errstate(over="ignore"):
        G = np.exp(-0.5 * q)
    return dx, dy, inside, G, np.minimum(u["op"][g][None, :] * G, STOP)


def forward64(case):
    """dict(C[H, W, 3], A, T, n_contrib, covered, excused): the composite in float64.  excused: a pixel one of whose decisions -- alpha >= 1/255
    at a record it composites, A > 0.99 at a record inside whose box it lies -- is within EXCUSE (relative) of its threshold."""
    W, H = case["W"], case["H"]
    u = _geometry(case)
    C, A = np.zeros((H, W, 3)), np.zeros((H, W))
    ncon = np.zeros((H, W), np.int64)
    covered, excused = np.zeros((H, W), bool), np.zeros((H, W), bool)
    limit = min(float(np.float32(case["point"] if case["point"] != 0.0 else 3.0)), effective_cap(case))
    for t in np.flatnonzero(case["ranges"][:-1] != EMPTY):
        g = forward_list(case, t)
        if g.size == 0:
            continue
        ys, xs = _tile_pixels(case, t)
        dx, dy, inside, _, alpha = _alpha(u, g, xs + 0.5, ys + 0.5)
        a, c, n, ex = np.zeros(ys.size), np.zeros((ys.size, 3)), np.zeros(ys.size, np.int64), np.zeros(ys.size, bool)
        for k in range(g.size):
            ins = inside[:, k]
            if case["mode"] == 0:   # point-cloud preview: yellow discs, no blending
                hit = ins & (dx[:, k] ** 2 + dy[:, k] ** 2 <= limit * limit)
                c[hit], a[hit], n[hit] = (1.0, 1.0, 0.0), 1.0, k + 1
                continue
            ex |= ins & (np.abs(a - STOP) <= EXCUSE * STOP)
            act = ins & ~(a > STOP)
            ex |= act & (np.abs(alpha[:, k] - MIN_ALPHA) <= EXCUSE * MIN_ALPHA)
            w = np.where(act, alpha[:, k] * (1.0 - a), 0.0)
            c += u["rgb"][g[k]][None, :] * w[:, None]
            a += w
            n = np.where(act & (alpha[:, k] >= MIN_ALPHA), k + 1, n)
        C[ys, xs], A[ys, xs], ncon[ys, xs], excused[ys, xs] = c, a, n, ex
        covered[ys, xs] = inside.any(1)
    return dict(C=C, A=A, T=1.0 - A, n_contrib=ncon, covered=covered, excused=excused)


def backward64(case, final_T, n_contrib, grad):
    """The analytic backward of the composite in float64, per (pixel, splat) over the first n_contrib entries of the pixel's tile list, summed
    per Gaussian and scaled by 1e6: (sums[N, 9], pairs[N], abs_sums[N, 9]) with the slots mean x y, conic x y z, opacity, r g b.  pairs counts
    the contributing (pixel, splat) pairs of a Gaussian (each is truncated to an integer by the kernels), abs_sums adds up absolute values."""
    u = _geometry(case)
    N = case["rows"].shape[0]
    sums, asums, pairs = np.zeros((N, 9)), np.zeros((N, 9)), np.zeros(N, np.int64)
    ranges, vals = case["ranges"], case["vals"]
    for t in np.flatnonzero(ranges[:-1] != EMPTY):
        start, end = int(ranges[t]), int(ranges[t + 1])
        entries = end - start if end > start else 0
        ys, xs = _tile_pixels(case, t)
        n = np.minimum(n_contrib[ys, xs].astype(np.int64), entries)
        E = int(n.max()) if n.size else 0
        if E == 0:
            continue
        g = vals[start:start + E].astype(np.int64)
        dx, dy, inside, G, alpha = _alpha(u, g, xs + 0.5, ys + 0.5)
        M = (np.arange(E)[None, :] < n[:, None]) & inside & (alpha >= MIN_ALPHA)
        om = np.where(M, 1.0 - alpha, 1.0)
        Tk = final_T[ys, xs].astype(np.float64)[:, None] / np.cumprod(om[:, ::-1], 1)[:, ::-1]   # the transmittance in front of entry k
        w = np.where(M, alpha * Tk, 0.0)
        gp = grad[ys, xs]                                                   # [P, 3]
        col = u["rgb"][g]                                                   # [E, 3]
        cw = col[None, :, :] * w[:, :, None]
        behind = np.cumsum(cw[:, ::-1], 1)[:, ::-1] - cw                    # sum_{j > k} c_j alpha_j T_j
        dLda = Tk * (col @ gp.T).T - np.einsum("pec,pc->pe", behind, gp) / (1.0 - alpha)
        dLdG = u["op"][g][None, :] * dLda
        c = u["conic"][g]
        parts = np.stack([dLdG * G * (c[None, :, 0] * dx + c[None, :, 1] * dy), dLdG * G * (c[None, :, 2] * dy + c[None, :, 1] * dx),
                          -0.5 * dLdG * G * dx * dx, -dLdG * G * dx * dy, -0.5 * dLdG * G * dy * dy, G * dLda,
                          w * gp[:, None, 0], w * gp[:, None, 1], w * gp[:, None, 2]], 2)
        parts = np.where(M[:, :, None], parts, 0.0) * FIXED
        np.add.at(sums, g, parts.sum(0))
        np.add.at(asums, g, np.abs(parts).sum(0))
        np.add.at(pairs, g, M.sum(0))
    return sums, pairs, asums


def reference_layout(sums9):
    """[N, 9] -> the reference's four arrays (means[2N], conics[4N] with slot 2 unused, opacity[N], colours[3N])."""
    n = sums9.shape[0]
    gc = np.zeros((n, 4), sums9.dtype)
    gc[:, 0], gc[:, 1], gc[:, 3] = sums9[:, 2], sums9[:, 3], sums9[:, 4]
    return sums9[:, 0:2].reshape(-1).copy(), gc.reshape(-1), sums9[:, 5].copy(), sums9[:, 6:9].reshape(-1).copy()


# ----------------------------------------------------------------------------- what a case reaches (the honesty checks)
def compacted_counts(case):
    """{(tile, block): [records K14 keeps per chunk of 64 list positions]}: the kernel's box-against-block test, restated."""
    u = _geometry(case)
    ntx = (case["W"] + 15) // 16
    out = {}
    for t in np.flatnonzero(case["ranges"][:-1] != EMPTY):
        start = int(case["ranges"][t])
        end = start
        while end < case["count"] and (int(case["keys"][end]) >> 16) == t + 1:
            end += 1
        v = case["vals"][start:end].astype(np.int64)
        ok = v < case["num_splats"]
        g = np.where(ok, v, 0)
        for sub in range(4):
            bx, by = 16 * (t % ntx) + 8 * (sub & 1), 16 * (t // ntx) + 8 * (sub >> 1)
            keep = ok & ~((bx + 0.5 - u["cx"][g] > u["ex"][g]) | (u["cx"][g] - (bx + 7.5) > u["ex"][g]) |
                          (by + 0.5 - u["cy"][g] > u["ey"][g]) | (u["cy"][g] - (by + 7.5) > u["ey"][g]))
            out[(int(t), sub)] = [int(keep[c:c + 64].sum()) for c in range(0, max(v.size, 1), 64)]
    return out


def block_cull(A, B, C, op, x0, x1, y0, y1):
    """blockcull.h's test in float64 (for the honesty check of family 6 only): (qmin, thr, margin) -- the kernel drops the record for the block
    when qmin > thr + margin; None where it keeps without computing (centre inside, or a conic that is not provably convex)."""
    if (x0 <= 0 <= x1 and y0 <= 0 <= y1) or not (A > 0 and C > 0 and A * C - B * B > 0):
        return None
    q = lambda dx, dy: A * dx * dx + 2 * B * dx * dy + C * dy * dy
    cl = lambda v, lo, hi: min(max(v, lo), hi)
    qmin = min(q(x0, cl(-B * x0 / C, y0, y1)), q(x1, cl(-B * x1 / C, y0, y1)), q(cl(-B * y0 / A, x0, x1), y0), q(cl(-B * y1 / A, x0, x1), y1))
    mx, my = max(abs(x0), abs(x1)), max(abs(y0), abs(y1))
    M = A * mx * mx + 2 * abs(B) * mx * my + C * my * my
    return qmin, 2.0 * np.log(255.0 * op), 1e-3 + 1e-5 * M


# ----------------------------------------------------------------------------- the families
BOX_SETS = ("none", "b0", "b1", "b2", "b3", "top", "bottom", "left", "right", "all")


def _box(s, which, tile, op=0.0123, conic=(FLAT, 0.0, FLAT)):
    """A splat whose extent box overlaps exactly the named blocks of `tile` (b0 b1 / b2 b3).  On a power-of-two viewport the box ends exactly
    on the outermost pixel centres (|d| == extent counts as inside); elsewhere it ends 0.4 px beyond them."""
    ox, oy = s.origin(tile)
    h, f = (3.5, 7.5) if s.exact else (3.9, 7.9)
    cx, cy, ex, ey = {"none": (-1.5, 4.0, 0.5, 0.5), "b0": (4, 4, h, h), "b1": (12, 4, h, h), "b2": (4, 12, h, h), "b3": (12, 12, h, h), "top": (8, 4, f, h),
                      "bottom": (8, 12, f, h), "left": (4, 8, h, f), "right": (12, 8, h, f), "all": (8, 8, f, f)}[which]
    if which == "none":   # left of the image (ndc -1.1: inside the domain), short of the first pixel centre
        return s.splat(-0.05 * s.W, min(oy + 4.0, s.H - 0.5), 0.25, 0.5, conic=conic, op=op)
    # (a ragged viewport's last tiles reach beyond the image: the centre stays inside the ndc range)
    cx, cy = min(ox + cx, 1.09 * s.W) - ox, min(oy + cy, 1.09 * s.H) - oy
    return s.splat(ox + cx, oy + cy, ex, ey, conic=conic, op=op)


def _family1():
    cases = []
    for W, H in ((16, 16), (9, 5), (17, 33)):
        for L in (0, 1, 2, 63, 64, 65, 127, 128, 129, 193):
            s = Scene(W, H)
            for t in range(s.T):
                if s.T > 1 and t == 1:
                    continue   # an empty tile among the others
                for i in range(L):
                    s.add(t, _box(s, BOX_SETS[(i * 7 + t) % 10], t))
            cases.append(s.case(f"list of {L} on {W}x{H}", 1))
    # the chunk table: per block and chunk the counts 64 / 0 / odd / even / 1 / 2, a middle chunk that keeps nothing, a block fed by the last chunk only
    s = Scene(16, 16)
    for i in range(193):
        c, l = divmod(i, 64)
        which = ("top" if l in (5, 10, 11) else "b0") if c == 0 else (("b3" if l in (7, 20, 33) else "none") if c == 1 else
                                                                     (("right" if l in (0, 21, 42, 63) else "none") if c == 2 else "all"))
        s.add(0, _box(s, which, 0))
    cases.append(s.case("chunk table", 1, claims=dict(counts={(0, 0): [64, 0, 0, 1], (0, 1): [3, 0, 4, 1], (0, 2): [0, 0, 0, 1], (0, 3): [0, 3, 4, 1]})))
    # two records in one block: the compacted count 2, and 1 next to it
    s = Scene(16, 16)
    for which in ("b2", "none", "bottom", "none", "none"):
        s.add(0, _box(s, which, 0, op=0.3))
    cases.append(s.case("counts one and two", 1, claims=dict(counts={(0, 2): [2], (0, 3): [1], (0, 0): [0]})))
    # several tiles: lists that end by key change mid-chunk, lists of exactly 64 and 128 entries followed by the next tile's, empty tiles before,
    # between and after, the last tile included
    for name, lens in (("key change mid-chunk", (0, 37, 0, 0, 70, 5, 0, 0)), ("full chunks then the next tile", (64, 3, 128, 1, 0, 64, 64, 0)),
                       ("only the last tile", (0, 0, 0, 0, 0, 0, 0, 9)), ("only the first tile", (130, 0, 0, 0, 0, 0, 0, 0))):
        s = Scene(64, 32)
        for t, L in enumerate(lens):
            for i in range(L):
                s.add(t, _box(s, BOX_SETS[1 + (i * 3 + t) % 9], t, op=0.02))
        cases.append(s.case(name, 1))
    # values >= num_splats: the table has three rows more than K14 is told (rows K16 and the reference's backward take as what they are)
    s = Scene(32, 16)
    real = [_box(s, BOX_SETS[1 + i % 9], i % 2, op=0.05) for i in range(140)]
    ghosts = [s.splat(8.0 + 3 * j, 8.0, 20.0, 20.0, op=0.05, rgb=(1.0, 0.0, 1.0)) for j in range(3)]
    l0 = [g for g in real if g % 2 == 0]
    l1 = [g for g in real if g % 2 == 1]
    for at, gh in ((0, ghosts[0]), (31, ghosts[1]), (64, ghosts[2]), (66, ghosts[0])):   # first of all, mid-chunk, first of the second chunk
        l0.insert(at, gh)
    l1.insert(69, ghosts[1])
    l1.append(ghosts[2])
    s.add(0, *l0)
    s.add(1, *l1)
    cases.append(s.case("values beyond num_splats", 1, num_splats=140, claims=dict(ghost_positions=True)))
    # a whole batch of 256 such values ends the walk, as it ends the reference's: the real entries behind it are never composited
    s = Scene(16, 16)
    front = [_box(s, "all", 0, op=0.05) for _ in range(3)]
    back = [_box(s, "all", 0, op=0.5) for _ in range(4)]
    gh = s.splat(8.0, 8.0, 20.0, 20.0, op=0.9)
    s.add(0, *(front + [gh] * (253 + 256) + back))
    cases.append(s.case("a batch of values beyond num_splats ends the walk", 1, num_splats=7, k16=False, claims=dict(forward_entries=3)))
    return cases


def _family2():
    cases = []
    for name, lead in (("saturates at a chunk's last record", 57), ("saturates one record into the next chunk", 58)):
        s = Scene(16, 16)
        for i in range(lead):
            s.add(0, _box(s, "none", 0))
        for i in range(7):
            s.add(0, _box(s, "all", 0, op=0.5))       # A = 1 - 2^-7 > 0.99 after the seventh, at every pixel
        for i in range(70):
            s.add(0, _box(s, "all", 0, op=0.25))      # behind the stop: never composited
        cases.append(s.case(name, 2, claims=dict(saturated_at=lead + 7, blocks=(0, 1, 2, 3))))
    s = Scene(16, 16)
    for i in range(7):
        s.add(0, _box(s, "b1", 0, op=0.5))
    for i in range(100):
        s.add(0, _box(s, "all", 0, op=0.0123))
    cases.append(s.case("one block saturated, its neighbours walk on", 2, claims=dict(saturated_at=7, blocks=(1,))))
    # A == 0.99 (not above it) and then alpha = 0.99: the smallest final T the forward pass can leave, 1e-4
    s = Scene(16, 16)
    for i in range(2):
        s.add(0, s.splat(8.5, 8.5, 6.0, 6.0, conic=(NARROW, 0.0, NARROW), op=1.0))
    s.add(0, _box(s, "all", 0, op=0.5))
    cases.append(s.case("smallest final T", 2, claims=dict(smallest_T_at=(8, 8))))
    # pixels of one block that saturate at different records: a staircase of half-transparent boxes, each one pixel column shorter
    s = Scene(16, 16)
    for i in range(96):   # columns 0..k and rows 0..k in turn, k running through 0..15 at two different paces
        k = 0.5 + ((i // 2) * 5 % 16 if i % 2 else (i // 2) * 3 % 16)
        op = (0.45, 0.3, 0.15)[i % 3]
        s.add(0, s.splat(0.0, 8.0, k, 7.5, op=op) if i % 2 else s.splat(8.0, 0.0, 7.5, k, op=op))
    cases.append(s.case("saturation staircase", 2, claims=dict(distinct_n_contrib=12)))
    return cases


def _family3():
    cases = []
    # opacity G across 1/255 and across 0.99: one narrow splat per tile, the opacity swept; the pixel ring at each distance has its own G
    for name, ops, conic in (("alpha across 1/255", (0.0079, 0.012, 0.02, 0.05, 0.1, 0.3, 0.7, 1.0), (0.25, 0.0, 0.25)),
                             ("alpha across 0.99", (0.98, 0.985, 0.99, 0.9902, 0.995, 1.0, 0.97, 0.9912), (0.004, 0.0, 0.004))):
        s = Scene(64, 32)
        for t, op in enumerate(ops):
            ox, oy = s.origin(t)
            s.add(t, s.splat(ox + 8.5, oy + 8.5, 12.0, 12.0, conic=conic, op=op), s.splat(ox + 4.0, oy + 6.0, 12.0, 12.0, conic=conic, op=op))
        cases.append(s.case(name, 3))
    # centred exactly on a pixel centre: G = 1, alpha = opacity; the opacity at the domain's lower end (the half above 1/128)
    s = Scene(16, 16)
    for i, op in enumerate((float(f16_step(1.0 / 128.0, 1)), 0.25, 1.0)):
        s.add(0, s.splat(2.5 + 5 * i, 8.5, 2.0, 2.0, conic=(1.0, 0.0, 1.0), op=op))
    cases.append(s.case("centred on a pixel, lowest opacity", 3))
    # alpha EQUAL to 1/255 in float32, at the pixel (8, 8) of each splat below: where `<` and `<=`, `>=` and `>` part
    s = Scene(16, 16)
    for a, c, dx, dy, op in EXACT_MIN_ALPHA:
        s.add(0, s.splat(8.5 - dx, 8.5 - dy, 20.0, 20.0, conic=(a, 0.0, c), op=op, rgb=(1.0, 0.5, 0.25)))
    cases.append(s.case("alpha equal to 1/255", 3, claims=dict(exact_min_alpha=(8, 8))))
    return cases


# (conic.x, conic.z, dx, dy, opacity) with float32(opacity * exp(-(conic.x dx^2 + conic.z dy^2) / 2)) == float32(1 / 255) under the kernels' pinned exp:
# conic and opacity are exact halves and conic.y = 0, so every product of the argument is exact and its sum is rounded once.  Found by a random
# search of a few million combinations; tests/test_raster_cases.py checks each one against the oracle's exp.
EXACT_MIN_ALPHA = ((0.21728515625, 0.256103515625, 4.5, 1.5, 0.047210693359375), (0.039215087890625, 0.013641357421875, 6.5, 6.5, 0.0119781494140625),
                   (0.01107025146484375, 0.8837890625, 4.5, -1.5, 0.0118560791015625))


def _family4():
    cases = []
    s = Scene(32, 32)
    e = 2.0
    for i, ext in enumerate((e, float(f16_step(e, -1)), float(f16_step(e, 1)), 0.0)):
        ox, oy = s.origin(i)
        s.add(i, s.splat(ox + 8.5, oy + 8.5, ext, ext, conic=(0.01, 0.0, 0.01), op=0.8))        # |d| = 2 exactly at the ring's pixels
        s.add(i, s.splat(ox + 4.5, oy + 4.0, ext, 0.5, conic=(0.01, 0.0, 0.01), op=0.6))        # centre between two pixel rows: |dy| = 0.5 exactly
    cases.append(s.case("extent equal to |d|, a half either side, zero", 4, claims=dict(ring=True)))
    for name, cap in (("extent above the cap, default cap", 0.0), ("extent above the cap, cap lifted", -1.0)):
        s = Scene(256, 16)
        a = s.splat(0.5, 8.5, 200.0, 200.0, op=0.4)
        b = s.splat(255.5, 4.0, 100.0, 1000.0, op=0.3)
        for t in range(s.T):
            s.add(t, a, b)
        cases.append(s.case(name, 4, cap=cap, lam=0.002, claims=dict(cap_edge=128)))   # (dx^2 reaches 65 000: a small lambda keeps a conic contribution inside i32)
    s = Scene(16, 16)
    for cx, cy in ((-1.5, 8.5), (17.5, 3.0), (8.0, -1.5), (6.0, 17.5), (-1.5, -1.5)):     # ndc +-1.1875: outside the image, inside the domain
        s.add(0, s.splat(cx, cy, 6.0, 6.0, conic=(0.05, 0.0, 0.05), op=0.7))
    cases.append(s.case("centres outside the image", 4))
    s = Scene(32, 32)
    for cx, cy in ((8.0, 8.0), (16.0, 16.0), (16.0, 4.5), (8.0, 16.0), (24.0, 24.0)):
        g = s.splat(cx, cy, 3.5, 4.5, conic=(0.1, 0.02, 0.1), op=0.6)
        for t in range(4):
            s.add(t, g)
    cases.append(s.case("centres on block and tile boundaries", 4))
    return cases


def _family5():
    cases = []
    s = Scene(32, 32)
    conics = ((FLAT, 0.0, FLAT), (NARROW, 0.0, NARROW), (3.0, 0.17, 0.01), (3.0, -0.17, 0.01), (0.01, 0.17, 3.0), (0.02, -0.1, 2.5))
    for i, c in enumerate(conics):
        g = s.splat(5.5 + 4 * i, 9.5 + 2 * i, 14.0, 14.0, conic=c, op=0.35)
        for t in range(4):
            s.add(t, g)
    cases.append(s.case("widest, narrowest, anisotropic of either sign", 5))
    # y rounded past sqrt(x z): argument 16 y - 16 at the pixel (+4, -4) -- 86.5, 87, 87.5 (and -119 at (-4, -4)); small extents keep it to that
    s = Scene(32, 32)
    for t, b in enumerate((6.40625, 6.4375, 6.46875, 1.0009765625)):
        ox, oy = s.origin(t)
        s.add(t, s.splat(ox + 8.5, oy + 8.5, 4.0, 4.0, conic=(1.0, b, 1.0), op=0.5), _box(s, "all", t, op=0.3))
        s.add(t, s.splat(ox + 4.5, oy + 4.5, 4.0, 4.0, conic=(1.0, -b, 1.0), op=0.0079))
    cases.append(s.case("indefinite conics: arguments 86.5, 87, 87.5", 5, f64_backward=False, claims=dict(arguments=((86.0, 87.0), (87.0, 87.0), (87.0, 88.0)))))
    # arguments around -80 and -86: -32 x at the pixels (+-8, 0)
    s = Scene(32, 32)
    for t, (a0, k) in enumerate(((2.5, 0), (2.5, 1), (2.5, -1), (2.6875, 0))):
        ox, oy = s.origin(t)
        a = float(f16_step(a0, k))
        s.add(t, s.splat(ox + 8.5, oy + 8.5, 9.0, 9.0, conic=(a, 0.0, a), op=1.0), _box(s, "all", t, op=0.2))
    s.add(3, s.splat(24.5, 24.5, 9.0, 9.0, conic=(float(f16_step(2.6875, 1)), 0.0, 0.5), op=1.0), s.splat(24.5, 24.5, 9.0, 9.0, conic=(float(f16_step(2.6875, -1)), 0.0, 0.5), op=1.0))
    cases.append(s.case("arguments around -80 and -86", 5, claims=dict(arguments=((-80.1, -80.0), (-80.0, -80.0), (-80.0, -79.9), (-86.1, -86.0), (-86.0, -86.0), (-86.0, -85.9)))))
    return cases


def _family6():
    """A few hundred splats whose largest alpha over one block's 64 pixel centres is within 2 % of 1/255, the centre outside the block."""
    rng = np.random.default_rng(606)
    s = Scene(32, 32)
    info = []
    deltas = (-0.02, -0.01, -0.004, -0.0015, -0.0005, 0.0005, 0.0015, 0.004, 0.01, 0.02)
    dirs = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))
    n = 0
    while len(info) < 320:
        n += 1
        blk = int(rng.integers(0, 16))
        bx, by = 8 * (blk % 4), 8 * (blk // 4)
        tile, sub = (by // 16) * 2 + bx // 16, ((by // 8) & 1) * 2 + ((bx // 8) & 1)
        ux, uy = dirs[n % 8]
        dist = float(rng.uniform(0.5, 5.0))
        on_row = bool(rng.integers(0, 2))
        # left / right / above / below: level with a pixel row (the nearest pixel is an edge pixel) or between rows; diagonal: off a corner
        cx = bx + (rng.integers(0, 8) + 0.5 if on_row else rng.uniform(0.5, 7.5)) if ux == 0 else (bx + 0.5 - dist if ux < 0 else bx + 7.5 + dist)
        cy = by + (rng.integers(0, 8) + 0.5 if on_row else rng.uniform(0.5, 7.5)) if uy == 0 else (by + 0.5 - dist * (1 if ux == 0 else rng.uniform(0.3, 1.0)) if uy < 0 else by + 7.5 + dist * (1 if ux == 0 else rng.uniform(0.3, 1.0)))
        cx, cy = float(np.clip(round(cx * 16) / 16, -3.0, 35.0)), float(np.clip(round(cy * 16) / 16, -3.0, 35.0))   # (exact in fp16 ndc at 32 px)
        kind = n % 3
        if kind == 0:
            a = float(rng.uniform(0.15, NARROW)); conic = (a, 0.0, a)
        else:   # anisotropic, the long axis along the direction to the block (kind 1) or across it (kind 2)
            th = np.arctan2(by + 4 - cy, bx + 4 - cx) + (0.0 if kind == 1 else np.pi / 2) + rng.normal(0, 0.15)
            l1, l2 = float(rng.uniform(0.03, 0.3)), float(rng.uniform(0.5, NARROW))      # eigenvalues of the conic: small along the long axis
            c_, s_ = np.cos(th), np.sin(th)
            conic = (l1 * c_ * c_ + l2 * s_ * s_, (l1 - l2) * c_ * s_, l1 * s_ * s_ + l2 * c_ * c_)
        conic = tuple(float(v) for v in f16v(conic))
        if not (conic[0] > 0 and conic[2] > 0 and conic[0] * conic[2] - conic[1] ** 2 > 1e-3):
            continue
        ys, xs = np.mgrid[by:by + 8, bx:bx + 8]
        dx, dy = xs + 0.5 - cx, ys + 0.5 - cy
        if np.abs(dx).min() == 0 and np.abs(dy).min() == 0:
            continue   # the centre is a pixel of the block
        Gmax = float(np.exp(-0.5 * (conic[0] * dx * dx + 2 * conic[1] * dx * dy + conic[2] * dy * dy)).max())
        op = float(f16v(MIN_ALPHA * (1.0 + deltas[n % 10]) / Gmax))
        if not (1.0 / 128.0 < op <= 1.0):
            continue
        g = s.splat(cx, cy, 40.0, 40.0, conic=conic, op=op)
        s.add(tile, g)
        info.append(dict(g=g, tile=tile, sub=sub, bx=bx, by=by))
    order = {t: rng.permutation(len(v)) for t, v in s.lists.items()}
    for t in s.lists:
        s.lists[t] = [s.lists[t][i] for i in order[t]]
    return [s.case("block cull at the 1/255 contour", 6, lam=4.0, claims=dict(cull=info))]


def _channel_images(W, H, channel=None, rows=None, cols=None, sign=None, value=200):
    """pred - targ = +-value in the chosen channel(s) and pixels, 0 elsewhere."""
    pred = np.zeros((H, W, 4), np.uint8)
    pred[:, :, 3] = 255
    targ = pred.copy()
    y, x = np.mgrid[0:H, 0:W]
    on = np.ones((H, W), bool)
    if rows is not None:
        on &= np.isin(y % 8, rows)
    if cols is not None:
        on &= np.isin(x % 8, cols)
    pos = on & ((sign(x, y) > 0) if sign else True)
    neg = on & ~pos
    for c in ([channel] if channel is not None else [0, 1, 2]):
        pred[:, :, c][pos], targ[:, :, c][neg] = value, value
    return pred, targ


def _family7():
    cases = []

    def scene(W=16, H=16, n=6, op=0.4, ext=30.0):
        s = Scene(W, H)
        gs = [s.splat(3.0 + 2.0 * i, 5.0 + 1.5 * i, ext, ext, conic=(0.02, 0.005 * (i % 3 - 1), 0.03), op=op) for i in range(n)]
        return s, gs

    s, gs = scene()
    s.add(0, *gs)
    pred, targ = _channel_images(16, 16, sign=lambda x, y: ((x + y) % 2) * 2 - 1)
    cases.append(s.case("contributions of both signs that cancel", 7, pred=pred, targ=targ))
    for name, lam in (("a pixel's contribution saturates the conversion", 3.0e7), ("sums wrap within a wave", 2000.0)):
        s, gs = scene()
        s.add(0, *gs)
        pred, targ = _channel_images(16, 16)
        cases.append(s.case(name, 7, pred=pred, targ=targ, lam=lam, f64_backward=False, claims=dict(wraps=True)))
    s, gs = scene(64, 32, n=4, ext=70.0)
    for t in range(8):
        s.add(t, *gs)
    pred, targ = _channel_images(64, 32)
    cases.append(s.case("sums wrap across the waves of several tiles", 7, pred=pred, targ=targ, lam=90.0, f64_backward=False, claims=dict(wraps_across=True)))
    for ch in range(3):
        s, gs = scene()
        s.add(0, *gs)
        pred, targ = _channel_images(16, 16, channel=ch, sign=lambda x, y: (x % 3 > 0) * 2 - 1)
        cases.append(s.case(f"gradient in channel {ch} only", 7, pred=pred, targ=targ, lam=3.0))
    for name, rows, cols in (("gradient in one 16-lane row", (2, 3), None), ("gradient in one 8-lane group", (5,), None), ("gradient in one pixel column", None, (6,))):
        s, gs = scene()
        s.add(0, *gs)
        pred, targ = _channel_images(16, 16, rows=rows, cols=cols)
        cases.append(s.case(name, 7, pred=pred, targ=targ, lam=2.0))
    # Gaussians that appear in no list, and lists that are not monotone in the Gaussian number
    s, gs = scene(32, 16, n=40, op=0.05)
    perm = np.random.default_rng(7).permutation(40)
    s.add(0, *[gs[i] for i in perm if i % 5])
    s.add(1, *[gs[i] for i in perm[::-1] if i % 5 and i % 3])
    cases.append(s.case("unlisted Gaussians, lists not monotone", 7, claims=dict(unlisted=[i for i in range(40) if i % 5 == 0])))
    return cases


def _family8(family1):
    cases = []
    for T in (1, 7, 8, 9, 17):
        s = Scene(16 * T, 16)
        for t in range(T):
            if T > 1 and t == T // 2:
                continue
            ox, _ = s.origin(t)
            for i in range(3 + t % 4):
                s.add(t, s.splat(ox + 3.0 + 3 * i, 4.0 + 2 * i, 5.9, 6.9, conic=(0.05, 0.01, 0.04), op=0.3 + 0.1 * (i % 3)))
        cases.append(s.case(f"{T} tiles", 8))
    s = Scene(16 * 2049, 16)
    for t in (0, 1, 1024, 2047, 2048):
        ox, _ = s.origin(t)
        for i in range(5):
            # (at this width an fp16 ndc centre is up to 8 px off: wide boxes and a wide conic, so that the tile is covered wherever it lands)
            s.add(t, s.splat(ox + 2.0 + 3 * i, 3.0 + 2 * i, 40.0, 40.0, conic=(0.002, 0.0005, 0.003), op=0.5))
    cases.append(s.case("2049 tiles in one row", 8))
    for L in (255, 256, 257, 300):
        s = Scene(16, 16)
        for i in range(L):
            s.add(0, _box(s, BOX_SETS[1 + i % 9], 0, op=0.02 if i < 250 else 0.4))
        cases.append(s.case(f"compat cap with {L} entries", 8, max_batches=1))
    for name in ("counts one and two", "key change mid-chunk"):
        base = next(c for c in family1 if c["name"] == name)
        cases.append(dict(base, name=name + ", point-cloud mode", family=8, mode=0, k16=False, point=2.0))
    return cases


_ALL = None


def all_cases():
    """Every case, built once and shared read-only."""
    global _ALL
    if _ALL is None:
        f1 = _family1()
        _ALL = tuple(f1 + _family2() + _family3() + _family4() + _family5() + _family6() + _family7() + _family8(f1))
        names = [c["name"] for c in _ALL]
        assert len(set(names)) == len(names)
    return _ALL


def family(n):
    return [c for c in all_cases() if c["family"] == n]
