"""Float64 restatement of the per-Gaussian render contribution, for the contribution tests.

The walk is ``depth64``'s: per pixel the records of its tile's list in order, a record *active* when the pixel is inside the image, ``|dx| <= ex``,
``|dy| <= ey`` and the running weight sum ``A`` is not ``> 0.99`` (box tests in float32 as the library forms them, everything else float64).  The
active pair's weight ``w = alpha (1 - A)`` is attributed to the record's Gaussian: summed, maximised, counted.

Saturation is the definition's one discontinuity: a float32 walk whose ``A`` falls on the other side of 0.99 at a step where the float64 ``A`` is within
``depth64.WINDOW`` of it goes on (or stops) where this one stops (or goes on).  Every later record of such a pixel is then in doubt, and what it can add
or drop is ``alpha (1 - A)`` with the ``A`` this walk holds there (frozen once saturated).  Those terms are the *slack* of the record's Gaussian.
"""
import numpy as np

import depth64 as d64
from depth64 import F99, WINDOW, _half


def contrib64(settings, tinfo, splats, ranges, sorted_keys, sorted_values, total_entries, max_entries=0):
    """dict of per-Gaussian float64 / int64 arrays: ``weight_sum``, ``max_weight``, ``pixels``; ``slack_sum``, ``slack_max``, ``slack_pixels`` (module
    docstring); ``surely_zero`` (bool): the Gaussian is in a list, and at every pixel of its box ``A - 0.99 > WINDOW`` before its record; ``in_list``.
    Also ``A`` (float64 ``[H, W]``), the pixels' final weight sums."""
    settings = np.asarray(settings, np.float32)
    vx, vy = settings[2], settings[3]
    W, H = int(vx), int(vy)
    cap = settings[6] if settings[6] > 0 else np.float32(1e9)
    ntx, total_tiles = int(tinfo[0]), int(tinfo[2])
    splats = np.asarray(splats, np.uint32).reshape(-1, 6)
    n = splats.shape[0]
    keys = np.asarray(sorted_keys, np.uint32)
    vals = np.asarray(sorted_values, np.uint32)
    total = int(total_entries)

    weight_sum = np.zeros(n); max_weight = np.zeros(n); pixels = np.zeros(n, np.int64)
    slack_sum = np.zeros(n); slack_max = np.zeros(n); slack_pixels = np.zeros(n, np.int64)
    in_list = np.zeros(n, bool); maybe_active = np.zeros(n, bool)
    A_img = np.zeros((H, W))

    cx_all = (_half(splats[:, 0], False) * np.float32(0.5) + np.float32(0.5)) * vx
    cy_all = (_half(splats[:, 0], True) * np.float32(-0.5) + np.float32(0.5)) * vy
    with np.errstate(invalid="ignore"):
        ex_raw, ey_raw = _half(splats[:, 1], False), _half(splats[:, 1], True)
        ex_all = np.where(cap < ex_raw, cap, ex_raw)
        ey_all = np.where(cap < ey_raw, cap, ey_raw)
    con_x = _half(splats[:, 2], False).astype(np.float64)
    con_y = _half(splats[:, 2], True).astype(np.float64)
    con_z = _half(splats[:, 3], False).astype(np.float64)
    opac = _half(splats[:, 5], True).astype(np.float64)

    lx, ly = np.meshgrid(np.arange(16), np.arange(16))
    for tile in range(total_tiles):
        start = int(ranges[tile])
        if start >= total:
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
        a = np.zeros(256)
        doubt = np.zeros(256, bool)   # a near-saturation step at an earlier record
        for e in range(start, end):
            g = int(vals[e])
            if g >= n:
                continue
            in_list[g] = True
            dx, dy = px - cx_all[g], py - cy_all[g]      # float32
            with np.errstate(invalid="ignore"):
                box = inside_image & ~(np.abs(dx) > ex_all[g]) & ~(np.abs(dy) > ey_all[g])
            if not box.any():
                continue
            # surely saturated before this record: A - 0.99 > WINDOW
            if np.any(box & ~(a - F99 > WINDOW)):
                maybe_active[g] = True
            active = box & ~(a > F99)
            if not (active.any() or (box & doubt).any()):
                continue
            dx64, dy64 = dx.astype(np.float64), dy.astype(np.float64)
            xe = -0.5 * (con_x[g] * dx64 * dx64 + 2.0 * con_y[g] * dx64 * dy64 + con_z[g] * dy64 * dy64)
            with np.errstate(over="ignore", under="ignore"):
                alpha = np.minimum(np.exp(xe) * opac[g], F99)
            term = alpha * (1.0 - a)
            d = box & doubt
            if d.any():
                slack_sum[g] += term[d].sum()
                slack_max[g] = max(slack_max[g], term[d].max())
                slack_pixels[g] += int(d.sum())
            if active.any():
                w = np.where(active, term, 0.0)
                weight_sum[g] += w.sum()
                max_weight[g] = max(max_weight[g], w.max())
                pixels[g] += int(active.sum())
                an = a + w
                doubt |= active & (np.abs(an - F99) < WINDOW)
                a = an
        ii = inside_image
        A_img[pyi[ii], pxi[ii]] = a[ii]
    return dict(weight_sum=weight_sum, max_weight=max_weight, pixels=pixels, slack_sum=slack_sum, slack_max=slack_max, slack_pixels=slack_pixels,
                surely_zero=in_list & ~maybe_active, in_list=in_list, A=A_img)
