"""Float64 numpy restatement of the exact D-SSIM loss (``dssim_mode="gaussian"``), written from its definition and sharing
no code with the kernel (``webdgs_amd/csrc/dssim.hip``).  Per view, with d = x - y, values u8/255 per rgb channel and S the SSIM map of
``ssim64`` (11x11 Gaussian window, sigma 1.5, zero padding, sigma^2 = E[x^2] - mu^2) with the given C1 and C2:

    L = sum over pixels and channels of  l1 |d| + l2 d^2 / 2 + ldssim (1 - S)

The loss image holds dL/dx per pixel and channel, plus w = 1.  The SSIM part is the textbook closed form: with A1 = 2 mx my + C1,
A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx^2 + sy^2 + C2, beta = dS/dsx^2 = -S/B2, gamma = dS/dsxy = 2 A1 / (B1 B2) and
a = S (2 my/A1 - 2 mx/B1) - 2 beta mx - gamma my,  dSum(S)/dx = w*a + 2 x (w*beta) + y (w*gamma)  (the maps 0 outside the image).
``tests/test_dssim_reference.py`` checks it against torch autograd of the 3DGS recipe and against finite differences."""
from __future__ import annotations

import numpy as np

from ssim64 import C1, C2, filter2d, rgb01, window1d


def _moments(x: np.ndarray, y: np.ndarray):
    g = window1d()
    mx, my = filter2d(x, g), filter2d(y, g)
    return g, mx, my, filter2d(x * x, g) - mx * mx, filter2d(y * y, g) - my * my, filter2d(x * y, g) - mx * my


def loss_value(x: np.ndarray, y: np.ndarray, lambda_l1=0.8, lambda_l2=0.0, lambda_dssim=0.2, c1=C1, c2=C2) -> float:
    """L for float images (3, H, W)."""
    _, mx, my, vx, vy, cxy = _moments(x, y)
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    d = x - y
    return float(np.sum(lambda_l1 * np.abs(d) + 0.5 * lambda_l2 * d * d + lambda_dssim * (1.0 - s)))


def ssim_sum_grad(x: np.ndarray, y: np.ndarray, c1=C1, c2=C2) -> np.ndarray:
    """d(sum of the SSIM map)/dx for float images (3, H, W)."""
    g, mx, my, vx, vy, cxy = _moments(x, y)
    a1, a2 = 2 * mx * my + c1, 2 * cxy + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    s = (a1 * a2) / (b1 * b2)
    beta = -s / b2
    gamma = 2 * a1 / (b1 * b2)
    a = s * (2 * my / a1 - 2 * mx / b1) - 2 * beta * mx - gamma * my
    return filter2d(a, g) + 2 * x * filter2d(beta, g) + y * filter2d(gamma, g)


def loss_grad(x: np.ndarray, y: np.ndarray, lambda_l1=0.8, lambda_l2=0.0, lambda_dssim=0.2, c1=C1, c2=C2) -> np.ndarray:
    """dL/dx for float images (3, H, W)."""
    d = x - y
    return lambda_l1 * np.sign(d) + lambda_l2 * d - lambda_dssim * ssim_sum_grad(x, y, c1, c2)


def loss_image(pred, targ, lambda_l1=0.8, lambda_l2=0.0, lambda_dssim=0.2, c1=C1, c2=C2) -> np.ndarray:
    """The loss image, (H, W, 4) float64, of rgba8 images ((H, W, 4) uint8 or (H, W) uint32)."""
    g = loss_grad(rgb01(pred), rgb01(targ), lambda_l1, lambda_l2, lambda_dssim, c1, c2)
    out = np.ones(g.shape[1:] + (4,), np.float64)
    out[..., :3] = np.moveaxis(g, 0, -1)
    return out
