"""The float64 restatement of the exact D-SSIM loss (tests/dssim64.py) against torch autograd of the 3DGS recipe and against finite
differences, its identities, and the host-side validation of ``dssim_mode``.  CPU only."""
import numpy as np
import pytest
import torch

import dssim64
import ssim64
from webdgs_amd import ops
from webdgs_amd.trainer import Trainer


def _torch_grad(a, b, lam, c1=ssim64.C1, c2=ssim64.C2) -> np.ndarray:
    """dL/dx by autograd of utils/loss_utils.py::ssim of the 3DGS code base in float64 (conv2d, padding 5, groups 3), L as dssim64 defines it."""
    import torch.nn.functional as F
    x = torch.from_numpy(ssim64.rgb01(a))[None].requires_grad_(True)
    y = torch.from_numpy(ssim64.rgb01(b))[None]
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] @ g[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    mx, my = conv(x), conv(y)
    vx, vy, cxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    r = x - y
    loss = (lam[0] * r.abs() + 0.5 * lam[1] * r * r + lam[2] * (1 - s)).sum()
    loss.backward()
    return x.grad[0].permute(1, 2, 0).numpy()


def _img(rng, h, w):
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("lam", [(0.8, 0.0, 0.2), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (11, 10), (17, 33), (40, 64)])
def test_matches_torch_autograd(h, w, lam):
    rng = np.random.default_rng(h * 100 + w)
    a = _img(rng, h, w)
    b = np.clip(a.astype(np.int32) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    got = dssim64.loss_image(a, b, *lam)
    want = _torch_grad(a, b, lam)
    assert got.shape == (h, w, 4) and np.all(got[..., 3] == 1.0)
    assert np.max(np.abs(got[..., :3] - want)) <= 1e-10


def test_matches_torch_autograd_flat_and_other_constants():
    """The cancelling case (bright and flat, variances far below C2) and a config's own C1, C2."""
    rng = np.random.default_rng(7)
    a = np.full((24, 20, 4), 255, np.uint8)
    b = (255 - rng.integers(0, 2, a.shape)).astype(np.uint8)
    assert np.max(np.abs(dssim64.loss_image(a, b) - np.concatenate([_torch_grad(a, b, (0.8, 0.0, 0.2)), np.ones((24, 20, 1))], -1))) <= 1e-10
    c = _img(rng, 13, 9)
    lam = (0.1, 0.2, 0.7)
    assert np.max(np.abs(dssim64.loss_image(a[:13, :9], c, *lam, c1=1e-3, c2=2e-3)[..., :3] - _torch_grad(a[:13, :9], c, lam, 1e-3, 2e-3))) <= 1e-10


def test_central_finite_differences():
    rng = np.random.default_rng(11)
    h, w = 14, 17
    x = ssim64.rgb01(_img(rng, h, w))
    y = ssim64.rgb01(_img(rng, h, w))
    lam = (0.8, 0.3, 0.6)
    grad = dssim64.loss_grad(x, y, *lam)
    eps = 1e-6
    for c, i, j in [(0, 0, 0), (1, 7, 8), (2, 13, 16), (0, 3, 15), (1, 12, 1), (2, 6, 6)]:
        assert abs(x[c, i, j] - y[c, i, j]) > 10 * eps   # (away from the kink of |d|)
        xp, xm = x.copy(), x.copy()
        xp[c, i, j] += eps
        xm[c, i, j] -= eps
        fd = (dssim64.loss_value(xp, y, *lam) - dssim64.loss_value(xm, y, *lam)) / (2 * eps)
        assert abs(fd - grad[c, i, j]) <= 1e-6 * max(1.0, abs(grad[c, i, j])), (c, i, j, fd, grad[c, i, j])


def test_identical_images_give_zero():
    rng = np.random.default_rng(3)
    for h, w in [(1, 1), (9, 13), (31, 23)]:
        a = _img(rng, h, w)
        g = dssim64.loss_image(a, a, 0.8, 0.5, 0.2)
        assert np.max(np.abs(g[..., :3])) <= 1e-9 and np.all(g[..., 3] == 1.0)


# ----------------------------------------------------------------------------- dssim_mode validation, no device
class _NoDevice:
    """Any use fails the test: validation has to happen before the first device call."""

    def __getattr__(self, name):
        raise AssertionError(f"device touched ({name})")


def test_dssim_mode_values():
    assert ops.dssim_mode(None) == 0 and ops.dssim_mode({}) == 0 and ops.dssim_mode(dict(dssim_mode=None)) == 0
    assert ops.dssim_mode(dict(dssim_mode="reference")) == 0
    assert ops.dssim_mode(dict(lambda_dssim=0.2, dssim_mode="gaussian")) == 1


@pytest.mark.parametrize("mode", ["box", "Gaussian", "", 1, True])
def test_ops_rejects_unknown_dssim_mode_without_a_device(mode):
    cfg = dict(viewportWidth=8, viewportHeight=8, trainingConfig=dict(lambda_dssim=0.2, dssim_mode=mode))
    with pytest.raises(ValueError):
        ops.TiledBackwardPass(_NoDevice(), _NoDevice(), cfg)
    # setTrainingConfig refuses it too, and keeps the config it had
    p = object.__new__(ops.TiledBackwardPass)
    p.device, p.handle, p.trainingConfig = _NoDevice(), None, dict(dssim_mode="gaussian")
    with pytest.raises(ValueError):
        p.setTrainingConfig(dict(dssim_mode=mode))
    assert p.trainingConfig == dict(dssim_mode="gaussian")


def test_trainer_rejects_unknown_dssim_mode_without_a_device():
    with pytest.raises(ValueError):
        Trainer(_NoDevice(), trainingConfig=dict(dssim_mode="ssim"))
