"""The float64 SSIM restatement (tests/ssim64.py) against the 3DGS recipe run through torch's conv2d in float64, and its own identities; the
held-out split convention.  CPU only."""
import math

import numpy as np
import pytest
import torch

import ssim64
from webdgs_amd import loaders


def _conv2d_ssim_map(a, b) -> np.ndarray:
    """utils/loss_utils.py::ssim of the 3DGS code base in float64: 2-D window = outer product of the 1-D Gaussian, padding 5, groups 3."""
    import torch.nn.functional as F
    x = torch.from_numpy(ssim64.rgb01(a))[None]
    y = torch.from_numpy(ssim64.rgb01(b))[None]
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    mx, my = conv(x), conv(y)
    vx, vy, cxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    m = ((2 * mx * my + ssim64.C1) * (2 * cxy + ssim64.C2)) / ((mx * mx + my * my + ssim64.C1) * (vx + vy + ssim64.C2))
    return m[0].permute(1, 2, 0).numpy()


def _img(rng, h, w):
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (11, 10), (17, 33), (40, 64)])
def test_matches_conv2d_recipe(h, w):
    rng = np.random.default_rng(h * 100 + w)
    a = _img(rng, h, w)
    b = np.clip(a.astype(np.int32) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    m64, mt = ssim64.ssim_map(a, b), _conv2d_ssim_map(a, b)
    assert m64.shape == (h, w, 3)
    assert np.max(np.abs(m64 - mt)) <= 1e-12
    assert abs(ssim64.ssim(a, b) - float(mt.mean())) <= 1e-12


def test_packed_u32_input_equals_rgba_bytes():
    rng = np.random.default_rng(1)
    a, b = _img(rng, 9, 13), _img(rng, 9, 13)
    assert ssim64.ssim(a.view(np.uint32)[..., 0], b.view(np.uint32)[..., 0]) == ssim64.ssim(a, b)


def test_identical_images_give_one():
    rng = np.random.default_rng(2)
    a = _img(rng, 23, 31)
    assert np.allclose(ssim64.ssim_map(a, a), 1.0, rtol=0, atol=1e-15)
    assert abs(ssim64.ssim(a, a) - 1.0) <= 1e-15


def test_symmetric():
    rng = np.random.default_rng(3)
    a, b = _img(rng, 19, 12), _img(rng, 19, 12)
    assert np.max(np.abs(ssim64.ssim_map(a, b) - ssim64.ssim_map(b, a))) <= 1e-15


def test_constant_images_interior():
    h, w, av, bv = 24, 30, 200, 90
    a = np.full((h, w, 4), av, np.uint8)
    b = np.full((h, w, 4), bv, np.uint8)
    m = ssim64.ssim_map(a, b)
    x, y = av / 255.0, bv / 255.0
    want = (2 * x * y + ssim64.C1) / (x * x + y * y + ssim64.C1)
    assert np.max(np.abs(m[5:-5, 5:-5] - want)) <= 1e-12
    # zero padding: the border sees the dark outside, so it is not the interior value
    assert abs(m[0, 0, 0] - want) > 1e-3


def test_window_is_normalised_gaussian():
    g = ssim64.window1d()
    assert len(g) == 11 and abs(g.sum() - 1.0) <= 1e-15 and np.argmax(g) == 5
    assert math.isclose(g[5] / g[6], math.exp(1.0 / (2 * 1.5 ** 2)), rel_tol=1e-13)


def test_holdout_split_every_8th():
    cams, imgs = [dict(id=i) for i in range(20)], [f"im{i}" for i in range(20)]
    trc, tri, tec, tei = loaders.holdoutSplit(cams, imgs)
    assert [c["id"] for c in tec] == [0, 8, 16] and tei == ["im0", "im8", "im16"]
    assert [c["id"] for c in trc] == [i for i in range(20) if i % 8] and tri == [f"im{i}" for i in range(20) if i % 8]
    trc, tri, tec, tei = loaders.holdoutSplit(cams[:5], imgs[:5], every=2)
    assert [c["id"] for c in tec] == [0, 2, 4] and [c["id"] for c in trc] == [1, 3]
    with pytest.raises(ValueError):
        loaders.holdoutSplit(cams, imgs[:3])
    with pytest.raises(ValueError):
        loaders.holdoutSplit(cams, imgs, every=0)
