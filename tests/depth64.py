"""Float64 restatement of the depth images' definition, for the depth tests.

For every pixel the records of its tile's sorted list are taken in order.  A record is *active* at the pixel when the pixel is inside the image,
``|dx| <= ex``, ``|dy| <= ey`` and the running weight sum ``A`` is not ``> 0.99``; then ``alpha = min(exp(xe) * opacity, 0.99)``,
``w = alpha (1 - A)``, ``A += w``, ``S += w z``; the median is the ``z`` of the first record at which ``A`` reaches 0.5.  The box tests, ``dx``,
``dy``, the centre and the extents are float32 as the library forms them from the Splat's fp16 fields (comparisons on exactly representable inputs
must fall as they do there); the exponent's argument, ``exp``, the weights and the sums are float64.  0.99 is the float32 nearest to it, as in the
library.  Written from the definition: one vector of a tile's 256 pixels, one loop over the tile's list.
"""
import numpy as np

WINDOW = 2e-6   # near_saturation / near_half: |A - threshold| below this at an active step
F99 = float(np.float32(0.99))


def decode_depths(depths_u32):
    """The inverse of the forward pass's order-preserving depth key: f32 view-space z per Gaussian."""
    u = np.asarray(depths_u32, np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u)
    return bits.astype(np.uint32).view(np.float32)


def _half(words, hi):
    w = np.asarray(words, np.uint32)
    return ((w >> np.uint32(16)) if hi else (w & np.uint32(0xFFFF))).astype(np.uint16).view(np.float16).astype(np.float32)


def depth64(settings, tinfo, splats, depths, ranges, sorted_keys, sorted_values, total_entries, max_entries=0, stats=None, probe=None):
    """``A``, ``D``, ``M`` as float64 ``[H, W]`` and the masks ``near_saturation``, ``near_half`` (module docstring).

    ``stats`` (a dict, optional) receives per pixel ``n_active`` (active records), ``z_min`` / ``z_max`` over them (+inf / -inf where none), and --
    with ``probe``, an ``[H, W]`` float32 image -- ``probe_in_box``: the probe's value at the pixel is the z of a record whose box holds the pixel."""
    settings = np.asarray(settings, np.float32)
    vx, vy = settings[2], settings[3]
    W, H = int(vx), int(vy)
    cap = settings[6] if settings[6] > 0 else np.float32(1e9)
    ntx, total_tiles = int(tinfo[0]), int(tinfo[2])
    splats = np.asarray(splats, np.uint32).reshape(-1, 6)
    n = splats.shape[0]
    z_all = decode_depths(depths)
    keys = np.asarray(sorted_keys, np.uint32)
    vals = np.asarray(sorted_values, np.uint32)
    total = int(total_entries)

    A = np.zeros((H, W)); S = np.zeros((H, W)); M = np.zeros((H, W))
    near_sat = np.zeros((H, W), bool); near_half = np.zeros((H, W), bool)
    n_active = np.zeros((H, W), np.int64)
    z_min = np.full((H, W), np.inf); z_max = np.full((H, W), -np.inf)
    in_box = np.zeros((H, W), bool)
    if probe is not None:
        probe = np.asarray(probe, np.float32)

    # the Splat's fields as the library unpacks them (float32 throughout)
    cx_all = (_half(splats[:, 0], False) * np.float32(0.5) + np.float32(0.5)) * vx
    cy_all = (_half(splats[:, 0], True) * np.float32(-0.5) + np.float32(0.5)) * vy
    with np.errstate(invalid="ignore"):
        ex_raw, ey_raw = _half(splats[:, 1], False), _half(splats[:, 1], True)
        ex_all = np.where(cap < ex_raw, cap, ex_raw)   # min(e, cap) that keeps a NaN extent
        ey_all = np.where(cap < ey_raw, cap, ey_raw)
    con_x = _half(splats[:, 2], False).astype(np.float64)
    con_y = _half(splats[:, 2], True).astype(np.float64)
    con_z = _half(splats[:, 3], False).astype(np.float64)
    opac = _half(splats[:, 5], True).astype(np.float64)

    lx, ly = np.meshgrid(np.arange(16), np.arange(16))
    for tile in range(total_tiles):
        start = int(ranges[tile])
        if start >= total:   # (0xFFFFFFFF: an empty tile)
            continue
        end = start
        limit = total if max_entries == 0 else min(total, start + int(max_entries))
        while end < limit and (int(keys[end]) >> 16) == tile + 1:
            end += 1
        tx, ty = tile % ntx, tile // ntx
        pxi, pyi = (tx * 16 + lx).reshape(-1), (ty * 16 + ly).reshape(-1)
        inside_image = (pxi < W) & (pyi < H)
        px = pxi.astype(np.float32) + np.float32(0.5)
        py = pyi.astype(np.float32) + np.float32(0.5)
        a = np.zeros(256); s = np.zeros(256); m = np.zeros(256)
        ns = np.zeros(256, bool); nh = np.zeros(256, bool); na = np.zeros(256, np.int64)
        zlo = np.full(256, np.inf); zhi = np.full(256, -np.inf); pb = np.zeros(256, bool)
        pv = None
        if probe is not None:
            pv = np.zeros(256, np.float32)
            pv[inside_image] = probe[pyi[inside_image], pxi[inside_image]]
        for e in range(start, end):
            g = int(vals[e])
            if g >= n:
                continue
            dx, dy = px - cx_all[g], py - cy_all[g]      # float32
            with np.errstate(invalid="ignore"):
                box = inside_image & ~(np.abs(dx) > ex_all[g]) & ~(np.abs(dy) > ey_all[g])
                if not box.any():
                    continue
                z = float(z_all[g])
                if pv is not None:
                    pb |= box & (pv == z_all[g])
                active = box & ~(a > F99)
                if not active.any():
                    continue
                dx64, dy64 = dx.astype(np.float64), dy.astype(np.float64)
                xe = -0.5 * (con_x[g] * dx64 * dx64 + 2.0 * con_y[g] * dx64 * dy64 + con_z[g] * dy64 * dy64)
                with np.errstate(over="ignore", under="ignore"):
                    alpha = np.minimum(np.exp(xe) * opac[g], F99)
                w = np.where(active, alpha * (1.0 - a), 0.0)
                an = a + w
                s = s + np.where(active, w * z, 0.0)
                m = np.where(active & (a < 0.5) & (an >= 0.5), z, m)
                ns |= active & (np.abs(an - F99) < WINDOW)
                nh |= active & (np.abs(an - 0.5) < WINDOW)
                a = an
            na += active
            zlo = np.where(active, np.minimum(zlo, z), zlo)
            zhi = np.where(active, np.maximum(zhi, z), zhi)
        ii = inside_image
        A[pyi[ii], pxi[ii]] = a[ii]; S[pyi[ii], pxi[ii]] = s[ii]; M[pyi[ii], pxi[ii]] = m[ii]
        near_sat[pyi[ii], pxi[ii]] = ns[ii]; near_half[pyi[ii], pxi[ii]] = nh[ii]
        n_active[pyi[ii], pxi[ii]] = na[ii]; z_min[pyi[ii], pxi[ii]] = zlo[ii]; z_max[pyi[ii], pxi[ii]] = zhi[ii]
        in_box[pyi[ii], pxi[ii]] = pb[ii]
    with np.errstate(invalid="ignore", divide="ignore"):
        D = np.where(A > 0, S / np.where(A > 0, A, 1.0), 0.0)
    if stats is not None:
        stats.update(n_active=n_active, z_min=z_min, z_max=z_max)
        if probe is not None:
            stats["probe_in_box"] = in_box
    return A, D, M, near_sat, near_half


def depth_to_rgba8_64(depth, near, far):
    """The presentation formula in float64: grey ``[H, W]`` uint8 and the float64 ``255 t`` it was rounded from (depth 0: grey 0)."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    near, far = float(np.float32(near)), float(np.float32(far))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (1.0 / d - 1.0 / far) / (1.0 / near - 1.0 / far)
    t = np.where(d != 0, np.clip(t, 0.0, 1.0), 0.0)
    v = 255.0 * t
    return np.floor(v + 0.5).astype(np.uint8), v
