"""Crafted images, tile lists and decision tables for the densify kernels (webdgs_amd/csrc/densify.hip), and a plain restatement of every stage.
Plain numpy: nothing here needs a GPU, the library or the oracle.

The restatements are integer where the stage is integer (cap, offsets, total, which output slot takes which source row, reset or carry) and
float64 where it is arithmetic (bilinear filter, L1 error, sigmoid, exp, per-pixel alpha, child positions).  tests/test_densify_cases.py holds
the oracle to them on exactly these inputs, tests/test_gpu_densify_kernels.py the kernels to the oracle.

Layouts: a Gaussian is 12 fp16 halves in 6 words (position 0-2, raw opacity 3, quaternion 4-7, log-scale 8-10, padding 11); a projected splat
is 12 halves in 6 words of which the metric count reads NDC centre 0-1, conic 4-6 and opacity 11; the optimizer state is the six arrays of
oracle.new_optimizer_state.
"""
import numpy as np

import indep64 as ind

SENTINEL = np.uint32(0xA5C3F00D)
STATE_WIDTHS = dict(opt_pos=12, opt_rot=12, opt_scale=12, opt_opacity=3, param_sh=48, state_sh=96)
LN_1P6 = 0.4700036292457356
OPACITY_MAX = float(np.float32(0.8))
OPACITY_MAX_RAW = np.float32(1.38629436112)
ALL_HALVES = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def f32(x):
    """The float32 a kernel argument becomes, as a Python float."""
    return float(np.float32(x))


def pack_halves(h16):
    """uint16 / float16 [n, 2k] -> u32 [n, k] (the first half of a pair is the low one)."""
    h = np.ascontiguousarray(h16)
    return h.view(np.uint16).view(np.uint32).reshape(h.shape[0], -1).copy()


def halves(words):
    w = np.ascontiguousarray(words, np.uint32)
    return w.view(np.uint16).reshape(w.shape[0], -1)


def pack_gaussians(pos, opacity, quat, log_scale):
    n = len(opacity)
    h = np.zeros((n, 12), np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        h[:, 0:3], h[:, 3], h[:, 4:8], h[:, 8:11] = pos, opacity, quat, log_scale
    return pack_halves(h)


# ===================================================================================================================== K31 down-sample
DOWNSAMPLE_SHAPES = (((37, 23), (16, 9)), ((5, 3), (17, 11)), ((64, 48), (64, 48)), ((1, 1), (4, 4)), ((100, 7), (33, 2)), ((33, 17), (11, 5)))
DOWNSAMPLE_BAND = 1e-3          # of a level, around a rounding boundary: float64 does not referee a texel inside it
DOWNSAMPLE_BAND_SHARE = 0.02


def downsample_id(shape):
    (sw, sh), (dw, dh) = shape
    return f"{sw}x{sh}-to-{dw}x{dh}"


def downsample_source(shape):
    (sw, sh), _ = shape
    return np.random.default_rng(3).integers(0, 256, (sh, sw, 4), dtype=np.uint8)


def downsample_fp64(src, dw, dh):
    """The linear sampler with clamp-to-edge addressing at destination texel centres, in levels (0..255), float64."""
    sh, sw = src.shape[:2]
    u = (np.arange(dw) + 0.5) / dw * sw - 0.5
    v = (np.arange(dh) + 0.5) / dh * sh - 0.5
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    wu, wv = (u - x0)[None, :, None], (v - y0)[:, None, None]
    cx, cy = (lambda a: np.clip(a, 0, sw - 1)), (lambda a: np.clip(a, 0, sh - 1))
    s = src.astype(np.float64)
    t00, t10 = s[cy(y0)][:, cx(x0)], s[cy(y0)][:, cx(x0 + 1)]
    t01, t11 = s[cy(y0 + 1)][:, cx(x0)], s[cy(y0 + 1)][:, cx(x0 + 1)]
    top, bot = t00 + (t10 - t00) * wu, t01 + (t11 - t01) * wu
    return top + (bot - top) * wv


# ===================================================================================================================== K21-K23 metric map
METRIC_SIZES = ((1, 1), (16, 16), (17, 33), (250, 130), (300, 250), (1024, 520))      # (width, height)
METRIC_CONTENTS = ("identical", "constant", "last-pixel", "random", "alpha-only")
METRIC_THRESHOLDS = (0.37, 0.0, 1.0)
METRIC_BAND = 1e-5


def metric_images(kind, w, h):
    rng = np.random.default_rng(17 + 31 * METRIC_CONTENTS.index(kind) + w)
    pred = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    targ = pred.copy()
    if kind == "constant":          # every pixel the same channel sum (9 + 0 + 20), signs mixed
        pred[..., :3] = np.clip(pred[..., :3], 20, 235)
        sign = np.where(rng.integers(0, 2, (h, w, 1)) == 0, -1, 1)
        targ[..., :3] = (pred[..., :3].astype(np.int64) + sign * np.array([9, 0, 20])).astype(np.uint8)
    elif kind == "last-pixel":
        targ[h - 1, w - 1, 1] ^= 0x40
    elif kind == "random":          # one pixel agrees, so that the smallest error is an exact 0 in any arithmetic
        targ = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        targ[h // 2, w // 3, :3] = pred[h // 2, w // 3, :3]
    elif kind == "alpha-only":
        targ[..., 3] = ~pred[..., 3]
    return pred, targ


def metric_exact(pred, targ, err_scale=1_000_000):
    """The stored error as exact integers: floor(err_scale * s / 765) with s the sum of the three channel differences."""
    s = np.abs(pred[..., :3].astype(np.int64) - targ[..., :3].astype(np.int64)).sum(-1)
    return (s * err_scale) // 765


def metric_flags_exact(err, threshold):
    """(flags, distance): the flag from the exact errors -- (e - min) > t (max - min) with t the float32 threshold, nothing flagged when
    max == min -- and |norm - t| per pixel."""
    mn, mx = int(err.min()), int(err.max())
    if mx == mn:
        return np.zeros(err.shape, np.uint32), np.full(err.shape, abs(0.0 - f32(threshold)))
    norm = (err - mn) / float(mx - mn)
    return (norm > f32(threshold)).astype(np.uint32), np.abs(norm - f32(threshold))


# ===================================================================================================================== K24 metric count
COUNT_N = 300
COUNT_VIEWPORTS = ((40, 24), (17, 33), (1, 1), (64, 64))
COUNT_LENGTHS = {(40, 24): (130, 63, 64, 65, 0, 1), (17, 33): (65, 1, 0, 130, 64, 63), (1, 1): (130,),
                 (64, 64): (63, 64, 65, 130, 0, 1, 63, 64, 65, 130, 0, 1, 63, 64, 65, 130)}
COUNT_FLAGS = ("all", "none", "checkerboard", "one-pixel", "random-70", "from-metric-map")
COUNT_OPACITIES = (0.0039, 0.004, 0.01, 0.3, 0.99, 1.0, 2.0, 0.0, -0.5)
COUNT_TAIL = 8                      # entries kept in memory after num_instances: a walk that does not stop there counts them
COUNT_NEAR = {(40, 24): 25, (17, 33): 25, (1, 1): 40, (64, 64): 12}      # a tile's list draws most entries from this many nearest Gaussians
N_MARGINAL = 12
COUNT_SEED = {(40, 24): 1, (17, 33): 3, (1, 1): 0, (64, 64): 2}     # chosen so that no pair outside the marginal family is within 1e-4 of the cut
MARGINAL_DELTAS = (0.004, -0.004, 0.015, -0.015)
_NONFINITE = (("cx", np.nan), ("cy", np.inf), ("cx", -np.inf), ("A", np.nan), ("A", np.inf), ("C", np.inf), ("B", np.nan), ("B", -np.inf),
              ("o", np.nan), ("o", np.inf), ("o", -np.inf))


def _conic(s1, s2, theta):
    c, s = np.cos(theta), np.sin(theta)
    a, b = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    return c * c * a + s * s * b, c * s * (a - b), s * s * a + c * c * b


def splat_fields(splats, W, H):
    """Float64 view of what the count reads of each record: pixel centre, conic, opacity (from the fp16 halves, exactly)."""
    with np.errstate(invalid="ignore"):
        h = halves(splats).view(np.float16).astype(np.float64)
        return dict(cx=(h[:, 0] * 0.5 + 0.5) * W, cy=(h[:, 1] * -0.5 + 0.5) * H, A=h[:, 4], B=h[:, 5], C=h[:, 6], o=h[:, 11])


def alpha255_fp64(f, ids, px, py):
    """255 * alpha of splats `ids` at pixels (px, py) (broadcast), alpha = min(0.99, o exp(-q / 2)) with a NaN taken as 0.99 -- both the
    kernel and the oracle write the minimum as `x < 0.99 ? x : 0.99`."""
    with np.errstate(all="ignore"):
        dx, dy = (px + 0.5) - f["cx"][ids], (py + 0.5) - f["cy"][ids]
        q = (f["A"][ids] * dx + 2.0 * f["B"][ids] * dy) * dx + (f["C"][ids] * dy) * dy
        og = f["o"][ids] * np.exp(-0.5 * q)
        return 255.0 * np.where(og < 0.99, og, 0.99)


def _marginal_splat(W, H, bx, by, kind, delta):
    """One record whose largest alpha over the pixels of the 8x8 block at (bx, by) is (1 + delta) / 255, from the ROUNDED centre and conic."""
    cx, cy = {"corner": (bx - 1.8, by - 1.2), "edge": (bx + 3.4, by - 2.1), "interior": (bx + 3.3, by + 4.4)}[kind]
    A, B, C = _conic(2.6, 1.9, 0.3)
    h = np.zeros((1, 12), np.float16)
    h[0, 0], h[0, 1], h[0, 4], h[0, 5], h[0, 6], h[0, 11] = 2.0 * cx / W - 1.0, 1.0 - 2.0 * cy / H, A, B, C, 0.5
    f = splat_fields(pack_halves(h), W, H)
    ys, xs = np.mgrid[by:by + 8, bx:bx + 8]
    a = alpha255_fp64(f, np.zeros(64, np.int64), xs.reshape(-1), ys.reshape(-1)) / 255.0 / 0.5      # = G (opacity 0.5 stays below the 0.99 cap)
    best = int(np.argmax(a))
    h[0, 11] = (1.0 + delta) / 255.0 / a[best]
    return h[0], (int(xs.reshape(-1)[best]), int(ys.reshape(-1)[best]))


def count_case(W, H):
    """Everything metric_count reads for one viewport, written here: `splats`, tile `ranges`, `instances` (num_instances entries and
    COUNT_TAIL more behind them), `n_contrib`, plus the `family` of every Gaussian and where the marginal ones attain their largest alpha."""
    n, rng = COUNT_N, np.random.default_rng(1000 * W + H + COUNT_SEED[(W, H)])
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    lengths = np.array(COUNT_LENGTHS[(W, H)], np.int64)
    assert lengths.size == ntx * nty and lengths[-1] > 0
    family = np.empty(n, "U9")
    h = rng.integers(0, 0x7C00, (n, 12)).astype(np.uint16).view(np.float16)      # the halves the kernel does not read: any finite value
    inside = rng.random(n) < 0.85
    # centres: most inside the viewport, the others up to 4 px past one of its edges
    cx = np.where(inside, rng.uniform(0, W, n), np.where(rng.random(n) < 0.5, -rng.uniform(0, 4, n), W + rng.uniform(0, 4, n)))
    cy = np.where(inside, rng.uniform(0, H, n), np.where(rng.random(n) < 0.5, -rng.uniform(0, 4, n), H + rng.uniform(0, 4, n)))
    s1 = np.exp(rng.uniform(np.log(0.6), np.log(6.0), n))
    s2, theta = s1.copy(), np.zeros(n)
    opacity = rng.choice([0.1, 0.3, 0.6, 0.99], n)
    family[:] = "iso"
    aniso = slice(132, 222)
    family[aniso] = "aniso"
    s2[aniso], theta[aniso] = np.exp(rng.uniform(np.log(0.6), np.log(6.0), 90)), rng.uniform(0, np.pi, 90)
    needle = slice(222, 242)
    family[needle] = "needle"
    s1[needle] = rng.uniform(3.0, 6.0, 20)
    s2[needle], theta[needle] = s1[needle] / rng.uniform(80.0, 400.0, 20), rng.uniform(0.3, 1.2, 20)
    opac = slice(242, 269)
    family[opac] = "opacity"
    s1[opac] = s2[opac] = rng.uniform(2.0, 4.0, 27)
    cx[opac], cy[opac] = rng.uniform(0, W, 27), rng.uniform(0, H, 27)
    opacity[opac] = np.resize(COUNT_OPACITIES, 27)
    A, B, C = _conic(s1, s2, theta)
    with np.errstate(over="ignore"):
        h[:, 0], h[:, 1], h[:, 4], h[:, 5], h[:, 6], h[:, 11] = 2.0 * cx / W - 1.0, 1.0 - 2.0 * cy / H, A, B, C, opacity
    nonfinite = np.arange(269, 269 + 2 * len(_NONFINITE))
    family[nonfinite] = "nonfinite"
    column = dict(cx=0, cy=1, A=4, B=5, C=6, o=11)
    for g, (field, value) in zip(nonfinite, _NONFINITE * 2):
        h[g, 11] = 0.3
        h[g, column[field]] = value

    # the marginal family, in the first fully visible tile whose list is long
    marginal, attain = np.zeros(0, np.int64), []
    tiles_ok = [t for t in range(ntx * nty) if lengths[t] >= 63 and (t % ntx) * 16 + 16 <= W and (t // ntx) * 16 + 16 <= H]
    mtile = tiles_ok[0] if tiles_ok else -1
    if mtile >= 0:
        marginal = np.arange(N_MARGINAL)
        for g in marginal:
            kind, delta = ("corner", "edge", "interior")[g % 3], MARGINAL_DELTAS[g // 3]
            bx, by = (mtile % ntx) * 16 + 8 * (g & 1), (mtile // ntx) * 16 + 8 * ((g >> 1) & 1)
            h[g], at = _marginal_splat(W, H, bx, by, kind, delta)
            attain.append((g, kind, delta, bx, by) + at)
        family[marginal] = "marginal"
    splats = pack_halves(h)

    # tile lists: 17 in 20 from the Gaussians nearest the tile, the rest from [0, n + 5); a Gaussian twice in every longer list
    f = splat_fields(splats, W, H)
    lists = []
    for t, L in enumerate(lengths):
        tx, ty = min((t % ntx) * 16 + 8, W - 0.5), min((t // ntx) * 16 + 8, H - 0.5)
        with np.errstate(invalid="ignore"):
            d = np.nan_to_num(np.hypot(f["cx"] - tx, f["cy"] - ty), nan=1e9, posinf=1e9)
        near = np.argsort(d, kind="stable")[:COUNT_NEAR[(W, H)]]
        k = (17 * L) // 20
        ids = np.concatenate([rng.choice(near, k), rng.integers(0, n + 5, L - k)])
        rng.shuffle(ids)
        if t == mtile:
            ids[:N_MARGINAL] = marginal
        if L >= 63:
            ids[40], ids[20], ids[50] = ids[30], ids[30], n + 2
        lists.append(ids)
    num_instances = int(lengths.sum())
    starts = np.concatenate([[0], np.cumsum(lengths)])
    ranges = np.where(np.append(lengths, 1) > 0, starts, 0xFFFFFFFF).astype(np.uint32)
    tail = rng.choice(near, COUNT_TAIL)
    instances = np.concatenate(lists + [tail]).astype(np.uint32)
    ys, xs = np.mgrid[0:H, 0:W]
    tile_of = (ys // 16) * ntx + xs // 16
    n_contrib = rng.integers(0, lengths[tile_of] + 9).astype(np.uint32)
    for (_, _, _, _, _, ax, ay) in attain:
        n_contrib[ay, ax] = max(int(n_contrib[ay, ax]), N_MARGINAL)
    n_contrib[H - 1, W - 1] = lengths[-1] + 8           # the last tile's walk runs past num_instances
    settings = np.array([1.0, 3.0, W, H, 3.0, 0.0, 128.0], np.float32)
    return dict(W=W, H=H, n=n, ntx=ntx, nty=nty, lengths=lengths, splats=splats, ranges=ranges, instances=instances, num_instances=num_instances,
                n_contrib=n_contrib, family=family, attain=attain, settings=settings, tile_of=tile_of)


def count_flags(kind, W, H):
    """The flag image of every kind but "from-metric-map" (that one is the metric map of `count_map_images` at threshold 0.37)."""
    ys, xs = np.mgrid[0:H, 0:W]
    if kind == "all":
        return np.ones((H, W), np.uint32)
    if kind == "none":
        return np.zeros((H, W), np.uint32)
    if kind == "checkerboard":
        return ((xs + ys) & 1).astype(np.uint32)
    if kind == "one-pixel":
        return ((xs == W // 2) & (ys == H // 2)).astype(np.uint32)
    assert kind == "random-70"
    return (np.random.default_rng(5 * W + H).random((H, W)) < 0.7).astype(np.uint32) * np.uint32(0x80000001)     # any non-zero word is a flag


def count_map_images(W, H):
    return metric_images("random", W, H)


def count_prefill(n, clear):
    """Counts before the call: garbage when the call clears them, small distinct values when it adds to them."""
    return np.full(n, SENTINEL, np.uint32) if clear else (np.arange(n, dtype=np.uint32) * 7 + 3)


def walked_pairs(case):
    """Every (pixel, Gaussian) pair the count may look at, flags aside: for each pixel the first min(n_contrib, num_instances - start) entries
    of its tile's list (none where the range word is 0xFFFFFFFF) whose Gaussian is below n.  Returns flat arrays (pixel, gaussian, 255 alpha)."""
    W, H, n, E = case["W"], case["H"], case["n"], case["num_instances"]
    f = splat_fields(case["splats"], W, H)
    pix, gid, a255 = [], [], []
    for t in range(case["ntx"] * case["nty"]):
        start = int(case["ranges"][t])
        if start == 0xFFFFFFFF:
            continue
        ys, xs = np.nonzero(case["tile_of"] == t)
        k = np.minimum(case["n_contrib"][ys, xs].astype(np.int64), max(E - start, 0))
        if k.size == 0 or k.max() == 0:
            continue
        ids = case["instances"][start:start + int(k.max())].astype(np.int64)
        valid = ids < n
        safe = np.where(valid, ids, 0)
        a = alpha255_fp64(f, safe[None, :], xs[:, None], ys[:, None])
        take = (np.arange(ids.size)[None, :] < k[:, None]) & valid[None, :]
        pix.append(np.broadcast_to((ys * W + xs)[:, None], take.shape)[take])
        gid.append(np.broadcast_to(safe[None, :], take.shape)[take])
        a255.append(a[take])
    if not pix:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(pix), np.concatenate(gid), np.concatenate(a255)


def count_bounds(case, pairs, flags, band=1e-4):
    """(low, high) per Gaussian: pairs of flagged pixels with alpha >= (1 + band) / 255, and with alpha >= (1 - band) / 255."""
    pix, gid, a = pairs
    on = flags.reshape(-1)[pix] != 0
    with np.errstate(invalid="ignore"):
        low = np.bincount(gid[on & ~(a < 1.0 + band)], minlength=case["n"])
        high = np.bincount(gid[on & ~(a < 1.0 - band)], minlength=case["n"])
    return low, high


# ===================================================================================================================== K25 normalize
NORMALIZE_SIZES = (1, 255, 256, 257)
NORMALIZE_DIVISORS = (1, 3, 0xFFFFFFFF, 0)


def normalize_counts(n):
    c = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c[::5], c[::7], c[::11] = 0xFFFFFFFF, 0, 0xFFFFFFFE
    c[n // 2] = 0 if n > 1 else 0xFFFFFFFF
    return c


def normalize_plain(counts, divisor):
    return (counts.astype(np.uint64) // max(1, int(divisor))).astype(np.uint32)


# ===================================================================================================================== K26 decide
DECIDE_PRUNE_THRESHOLDS = (0.15, 0.01)
DECIDE_SPLIT_THRESHOLDS = (0.012, 0.05, 1.0, 2.5)
DECIDE_CLONE_THRESHOLD = 6


def decide_opacity_sweep():
    """One Gaussian per fp16 pattern as raw opacity; tiny scales (a clone never becomes a split); the counts walk the edges of the threshold."""
    n = 65536
    g = pack_gaussians(np.zeros((n, 3)), np.zeros(n), np.tile([1.0, 0, 0, 0], (n, 1)), np.full((n, 3), -10.0))
    hv = halves(g).copy()
    hv[:, 3] = ALL_HALVES
    t = DECIDE_CLONE_THRESHOLD
    counts = np.resize(np.array([t - 1, t, t + 1, 0, 0xFFFFFFFF], np.uint32), n)
    return pack_halves(hv), counts


def decide_scale_sweep(axis):
    """One Gaussian per fp16 pattern as log-scale `axis`, the two others at -10; kept by opacity, cloned or split by count."""
    n = 65536
    g = pack_gaussians(np.zeros((n, 3)), np.zeros(n), np.tile([1.0, 0, 0, 0], (n, 1)), np.full((n, 3), -10.0))
    hv = halves(g).copy()
    hv[:, 8 + axis] = ALL_HALVES
    return pack_halves(hv), np.full(n, DECIDE_CLONE_THRESHOLD, np.uint32)


def decide_plain(g, metric_counts, clone_threshold, prune_opacity, split_scale):
    """(counts, actions) in float64: prune (3, 0) below the opacity threshold, else clone (1, 2) or split (2, 2) at the count threshold by
    the largest scale, else keep (0, 1).  A NaN compares false everywhere, as in the shader."""
    gs = ind.unpack_gaussians(g)
    with np.errstate(over="ignore", invalid="ignore"):
        prune = ind.sigmoid(gs["opacity_raw"]) < f32(prune_opacity)
        big = (np.exp(gs["log_scale"]) >= f32(split_scale)).any(1)
    mc = np.zeros(g.shape[0], np.uint32) if metric_counts is None else metric_counts
    grow = mc.astype(np.int64) >= int(clone_threshold)
    actions = np.where(prune, 3, np.where(grow, np.where(big, 2, 1), 0)).astype(np.uint32)
    counts = np.where(prune, 0, np.where(grow, 2, 1)).astype(np.uint32)
    return counts, actions


# ===================================================================================================================== K27-K28 cap, scans, total
CAP_SIZES = (1, 64, 257, 4097)


def exclusive_scan(counts):
    c = counts.astype(np.uint64)
    return ((np.cumsum(c) - c) & 0xFFFFFFFF).astype(np.uint32)


def cap_cloud(n):
    """A cloud whose decision (clone threshold 6, prune 0.15, split 0.05) mixes counts 0, 1 and 2, with its metric counts."""
    rng = np.random.default_rng(40 + n)
    kind = rng.integers(0, 4, n) if n > 1 else np.array([2])        # 0 prune, 1 keep, 2 clone, 3 split
    g = pack_gaussians(rng.normal(0, 1, (n, 3)), np.where(kind == 0, -6.0, 0.5), np.tile([1.0, 0, 0, 0], (n, 1)),
                       np.where(kind == 3, -1.0, -6.0)[:, None] * np.ones((1, 3)))
    return g, np.where(kind >= 2, 9, 2).astype(np.uint32), kind


def cap_plain(counts, actions, max_out):
    """The cap on decided counts, integers: what starts at or past max_out is dropped; a pair whose first slot is the last one becomes a keep."""
    off = exclusive_scan(counts).astype(np.int64)
    drop = (max_out == 0) | (off >= max_out)
    half = ~drop & (counts == 2) & (off == max_out - 1)
    c = np.where(drop, 0, np.where(half, 1, counts)).astype(np.uint32)
    a = np.where(drop, 3, np.where(half, 0, actions)).astype(np.uint32)
    o = exclusive_scan(c)
    total = int((int(o[-1]) + int(c[-1])) & 0xFFFFFFFF) if c.size else 0
    return c, a, o, total


def cap_values(counts):
    """name -> maxOutPoints for one decided count array (names without a value for this array are left out)."""
    off = exclusive_scan(counts).astype(np.int64)
    total = int(counts.sum())
    v = {"0": 0, "1": 1, "2": 2, "total": total, "total+1": total + 1, "max": 0xFFFFFFFF}
    pairs, singles = np.flatnonzero(counts == 2), np.flatnonzero(counts == 1)
    if pairs.size:
        v["pair-first-slot"] = int(off[pairs[pairs.size // 2]]) + 1
    if singles.size:
        v["single"] = int(off[singles[singles.size // 2]]) + 1
    return v


def max_out_plain(n, max_buffer_bytes, max_new_points):
    m = 2 * max(n, 1)
    if max_buffer_bytes:
        m = min(max_buffer_bytes // 24, max_buffer_bytes // 96)
    if max_new_points > 0:
        m = min(m, max(n, 1) + max_new_points)
    return min(m, 0xFFFFFFFF)


# ===================================================================================================================== K29 + K30 scatter
SCATTER_SIZES = (1, 63, 64, 65, 257, 1000, 5000)       # at 5000 the seeds' src * 1664525 and src * 747796405 wrap
SCATTER_CASES = tuple(("mixed", n) for n in SCATTER_SIZES) + (("waves", 357), ("short", 257), ("short", 1000), ("long", 65), ("long", 1000),
                                                               ("odd", 1), ("odd", 257), ("odd", 1000), ("odd", 5000))
_ARRAYS = tuple(STATE_WIDTHS)


def provenance_state(n, rows=None):
    """State arrays in which every float names (array, source row, column): an integer below 2^23, exact in float32."""
    rows = np.arange(n) if rows is None else rows
    return {k: ((a * 128 + np.arange(w)[None, :]) * 8192 + rows[:, None] + 1).astype(np.float32) for a, (k, w) in enumerate(STATE_WIDTHS.items())}


def provenance_sh(n):
    return (np.uint32(0x70000000) | (np.arange(24, dtype=np.uint32)[None, :] << 20) | np.arange(n, dtype=np.uint32)[:, None]).astype(np.uint32)


def scatter_cloud(n, seed=0):
    """A cloud and optimizer state for the scatter: parameters random (opacities on both sides of the 0.8 clamp), moments / SH rows provenance;
    the fp32 masters are the fp16 values plus a little, so a child computed from the wrong copy shows."""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    q = rng.normal(0, 1, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g = pack_gaussians(rng.normal(0, 2, (n, 3)), rng.uniform(-4, 4, n), q, rng.uniform(-5, -1, (n, 3)))
    gs = ind.unpack_gaussians(g)
    st = provenance_state(n)
    st["opt_pos"][:, 0:3] = gs["pos"] + rng.normal(0, 1e-3, (n, 3))
    st["opt_rot"][:, 0:4] = gs["quat"] + rng.normal(0, 1e-4, (n, 4))
    st["opt_scale"][:, 0:3] = gs["log_scale"] + rng.normal(0, 1e-3, (n, 3))
    st["opt_opacity"][:, 0] = gs["opacity_raw"] + rng.normal(0, 1e-3, n)
    return g, provenance_sh(n), st


def _tables_from_kinds(kind):
    """kind per Gaussian: 0 drop, 1 keep, 2 clone, 3 split -> (counts, actions, offsets) as a prepare would leave them."""
    counts = np.array([0, 1, 2, 2], np.uint32)[kind]
    actions = np.array([3, 0, 1, 2], np.uint32)[kind]
    return counts, actions, exclusive_scan(counts)


def scatter_tables(name, n):
    """(counts, actions, offsets, out_n) of the named table shape."""
    rng = np.random.default_rng(900 + n)
    kind = rng.integers(0, 4, n)
    if name == "mixed":
        kind[n // 2] = 3
    elif name == "waves":          # wave 0 nothing, wave 1 all splits, wave 2 lane 0 only, wave 3 lane 63 only, the rest mixed
        assert n >= 5 * 64 + 1
        kind[0:64], kind[64:128], kind[128:256] = 0, 3, 0
        kind[128], kind[255] = 2, 3
    counts, actions, offsets = _tables_from_kinds(kind)
    total = int(counts.sum())
    if name in ("mixed", "waves"):
        return counts, actions, offsets, max(total, 1)
    if name == "short":            # the output ends between the two children of a pair
        pairs = np.flatnonzero(counts == 2)
        return counts, actions, offsets, int(offsets[pairs[pairs.size // 2]]) + 1
    if name == "long":
        return counts, actions, offsets, total + 7
    assert name == "odd"
    # tables no prepare would write: holes between the rows, offsets at and past the end, counts 3 and 0xFFFFFFFF (one slot each),
    # a pair whose action is "keep", a single whose action is "prune", an action above 3
    i = np.arange(n)
    counts = np.where(i % 11 == 3, 3, np.where(i % 11 == 7, 0xFFFFFFFF, counts)).astype(np.uint32)
    actions = np.where((i % 5 == 1) & (counts == 2), 0, np.where((i % 5 == 2) & (counts == 1), 3, np.where(i % 13 == 4, 7, actions))).astype(np.uint32)
    slots = np.where(counts == 0, 0, np.where(counts == 2, 2, 1)).astype(np.uint32)
    offsets = (exclusive_scan(slots).astype(np.int64) + np.cumsum(rng.integers(0, 3, n))).astype(np.uint32)
    out_n = int(offsets[(3 * n) // 4]) + 1 if n > 1 else 4
    if n > 8:
        offsets[n - 1], offsets[n - 2], offsets[n - 3] = 0xFFFFFFFF, out_n, 0x80000000
    return counts, actions, offsets, out_n


def scatter_plan(counts, offsets, out_n):
    """Which output slot takes which source row, integers: (dst, src, variant).  A row with a non-zero count whose offset is inside the
    output gives slot `offset`; a count of exactly 2 also gives `offset + 1` if that is inside.  No two rows may name one slot."""
    off = offsets.astype(np.int64)
    live = (counts != 0) & (off < out_n)
    two = live & (counts == 2) & (off + 1 < out_n)
    s0, s1 = np.flatnonzero(live), np.flatnonzero(two)
    dst, src = np.concatenate([off[s0], off[s1] + 1]), np.concatenate([s0, s1])
    variant = np.concatenate([np.zeros(s0.size, np.int64), np.ones(s1.size, np.int64)])
    assert np.unique(dst).size == dst.size, "two rows write one slot"
    order = np.argsort(dst)
    return dst[order], src[order], variant[order]


def value_cloud():
    """The value edges of the scatter, one Gaussian per combination that matters, all as splits, clones and keeps (`value_tables`): master
    opacities on a ladder of +-8 float32 neighbours around the clamp value plus +-inf and NaN; log-scales beyond the +-10 clamp (+-11, +-65504, inf,
    NaN); a zero quaternion, lengths 1e-3 and 100, a NaN component; positions 0 and 6e4, where a child overflows fp16."""
    ladder = [np.float32(OPACITY_MAX_RAW)]
    for _ in range(8):
        ladder = [np.nextafter(ladder[0], np.float32(-np.inf))] + ladder + [np.nextafter(ladder[-1], np.float32(np.inf))]
    opac = np.array(ladder + [np.inf, -np.inf, np.nan, 0.0], np.float32)
    scales = np.array([[-2, -2, -2], [11, -2, -2], [-2, -11, -2], [65504, -2, -2], [-2, -2, -65504], [np.inf, -2, -2], [-2, -np.inf, -2], [-2, np.nan, -2]], np.float64)
    quats = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [1e-3, 0, 0, 0], [0, 6e-4, 8e-4, 0], [60, 0, 80, 0], [np.nan, 1, 0, 0], [0.5, 0.5, -0.5, 0.5]], np.float64)
    poss = np.array([[0, 0, 0], [6e4, -6e4, 6e4], [1.5, -2.5, 3.5]], np.float64)
    rows = []
    for i in range(len(opac)):
        rows.append((i, 0, 6, 2))
    for s in range(len(scales)):
        for q in range(len(quats)):
            for p in range(len(poss)):
                rows.append((len(opac) - 1, s, q, p))
    rows = np.array(rows)
    n = rows.shape[0]
    o, s, q, p = opac[rows[:, 0]], scales[rows[:, 1]], quats[rows[:, 2]], poss[rows[:, 3]]
    g = pack_gaussians(p, o, q, s)
    st = provenance_state(n)
    st["opt_pos"][:, 0:3], st["opt_rot"][:, 0:4], st["opt_scale"][:, 0:3], st["opt_opacity"][:, 0] = p, q, s, o
    return g, provenance_sh(n), st


def value_tables(n, what):
    """Every Gaussian kept (1 slot), cloned or split (2 slots each)."""
    kind = np.full(n, {"keep": 1, "clone": 2, "split": 3}[what])
    counts, actions, offsets = _tables_from_kinds(kind)
    return counts, actions, offsets, int(counts.sum())


def opacity_sweep_cloud():
    """Every fp16 pattern as raw opacity, n = 65 536; the masters hold the fp16 values."""
    n = 65536
    rng = np.random.default_rng(77)
    q = rng.normal(0, 1, (n, 4))
    g = pack_gaussians(rng.normal(0, 2, (n, 3)), np.zeros(n), q, rng.uniform(-5, -1, (n, 3)))
    hv = halves(g).copy()
    hv[:, 3] = ALL_HALVES
    g = pack_halves(hv)
    gs, st = ind.unpack_gaussians(g), provenance_state(n)
    with np.errstate(invalid="ignore"):
        st["opt_pos"][:, 0:3], st["opt_rot"][:, 0:4], st["opt_scale"][:, 0:3], st["opt_opacity"][:, 0] = gs["pos"], gs["quat"], gs["log_scale"], gs["opacity_raw"]
    return g, provenance_sh(n), st


# ---- the children (moved here from test_oracle_independent.py)
def _rand01(seed_u32):
    """f32(hash) * 2^-32 (densify-prune-scatter-gaussians.wgsl:40-43): the u32 -> f32 conversion rounds to 24 bits."""
    return ind.lowbias32(seed_u32).astype(np.float32).astype(np.float64) / 4294967296.0


def _densify_children_fp64(pos, quat, log_sigma, src, dst, action, variant):
    """Child position and log-scale of output slot `dst` copied from input `src` (float64, vectorised): clone slot 1 is jittered by
    0.25 sigma (.) U(-1,1)^3, split children sit at +- 0.5 sigma (.) n with n a six-uniform CLT normal and shrink by ln 1.6; offsets are
    rotated by the (normalised) quaternion (densify-prune-scatter-gaussians.wgsl:79-150)."""
    src32, dst32 = src.astype(np.uint64), dst.astype(np.uint64)
    sigma = np.exp(np.clip(log_sigma, -10, 10))
    R = ind.rotation_from_quaternion(quat / np.sqrt(np.maximum(1e-12, (quat * quat).sum(1, keepdims=True))))
    out_pos, out_ls = pos.copy(), log_sigma.copy()
    clone = (action == 1) & (variant == 1)
    seed = ((src32 * 1664525 + dst32 * 1013904223) & 0xFFFFFFFF).astype(np.uint64)
    r = np.stack([_rand01(seed ^ c) for c in (0xA2C79, 0x5E2D9, 0x1B873)], 1) * 2.0 - 1.0
    out_pos[clone] += np.einsum("nij,nj->ni", R, 0.25 * sigma * r)[clone]
    split = action == 2
    seed2 = ((src32 * 747796405 + 2891336453) & 0xFFFFFFFF).astype(np.uint64)

    def randn(s):
        return (sum(_rand01(s ^ c) for c in (0xA2C79, 0x5E2D9, 0x1B873, 0xC0FFE, 0xBADC0, 0xDEADB)) - 3.0) * 1.41421356237
    d = np.stack([randn(seed2 ^ c) for c in (0x9E3779B9, 0x243F6A88, 0xB7E15162)], 1)
    sgn = np.where(variant == 1, -1.0, 1.0)[:, None]
    out_pos[split] += (sgn * np.einsum("nij,nj->ni", R, 0.5 * sigma * d))[split]
    out_ls[split] = np.clip(log_sigma, -10, 10)[split] - 0.4700036292457356
    return out_pos, out_ls
