"""Crafted rgba8 image pairs for the loss-image tests, CPU and GPU: the four kinds of tests/test_gpu_eval.py (noise, smooth, flat, identical) and two
that rendered pairs never produce -- windows whose covariance is negative, and saturated differences that reach an image edge."""
import numpy as np

from test_gpu_eval import KINDS as EVAL_KINDS, _pair as _eval_pair

KINDS = EVAL_KINDS + ["anti", "saturated"]


def pair(kind, w, h, seed):
    """(a, b), uint8 [h, w, 4], for every w, h >= 1.

    anti       a one-pixel checkerboard of 0 / 255 in RGB against its inverse, alpha 255: every 5x5 window has covariance -variance, SSIM near -1.
    saturated  a = 0 against b = 255 in the top half (the upper ceil(h / 2) rows), 255 against 0 below, alpha 255; the two left-most columns of b
               are a's, so the difference is 0 (sign(0) = 0) on an image edge whose clamp-to-edge halo repeats the equal columns."""
    if kind == "anti":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.full((h, w, 4), 255, np.uint8)
        a[..., :3] = (((xx + yy) & 1) * 255).astype(np.uint8)[..., None]
        b = a.copy()
        b[..., :3] = 255 - a[..., :3]
        return a, b
    if kind == "saturated":
        top = (h + 1) // 2
        a, b = np.full((h, w, 4), 255, np.uint8), np.full((h, w, 4), 255, np.uint8)
        a[:top, :, :3], b[top:, :, :3] = 0, 0
        b[:, :2, :3] = a[:, :2, :3]
        return a, b
    return _eval_pair(kind, w, h, seed)
