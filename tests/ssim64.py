"""Float64 numpy SSIM, written from the definition (Wang et al. 2004) with the conventions of the 3DGS code base's ``ssim``: values u8/255 per rgb
channel, an 11x11 Gaussian window (sigma 1.5, normalised to sum 1), zero padding, C1 = 0.01^2, C2 = 0.03^2, sigma^2 = E[x^2] - mu^2.  Whole
arrays at a time, no shift, no shared code with the kernel (``webdgs_amd/csrc/ssim.hip``).  The window is applied as two 1-D passes -- the 2-D
window is the outer product of the 1-D one -- which ``tests/test_ssim_reference.py`` checks against a 2-D ``conv2d`` in float64."""
from __future__ import annotations

import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2
RADIUS, SIGMA = 5, 1.5


def window1d(radius: int = RADIUS, sigma: float = SIGMA) -> np.ndarray:
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return g / g.sum()


def rgb01(img) -> np.ndarray:
    """(H, W, 4) uint8 rgba, or (H, W) uint32 packed rgba8 -> (3, H, W) float64 in [0, 1]."""
    a = np.asarray(img)
    if a.dtype == np.uint32:
        a = a.view(np.uint8).reshape(a.shape + (4,))
    return np.moveaxis(a[..., :3].astype(np.float64) / 255.0, -1, 0)


def filter2d(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """Separable correlation of (..., H, W) with the window g x g, zero padding, same size out."""
    r = len(g) // 2
    h, w = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)])
    rows = sum(g[k] * p[..., :, k:k + w] for k in range(len(g)))
    return sum(g[k] * rows[..., k:k + h, :] for k in range(len(g)))


def ssim_map(a, b) -> np.ndarray:
    """The per-pixel, per-channel SSIM map, (H, W, 3) float64."""
    x, y = rgb01(a), rgb01(b)
    g = window1d()
    mx, my = filter2d(x, g), filter2d(y, g)
    vx = filter2d(x * x, g) - mx * mx
    vy = filter2d(y * y, g) - my * my
    cxy = filter2d(x * y, g) - mx * my
    m = ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return np.moveaxis(m, 0, -1)


def ssim(a, b) -> float:
    """Mean of the map over 3 W H values."""
    return float(ssim_map(a, b).mean())
