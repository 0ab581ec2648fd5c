"""GPU: the reference-mode loss kernel (csrc/loss.hip, the default dssim_mode) on crafted image pairs, bit for bit against the oracle's K15, in both of
its launch forms (one pixel per thread up to 640 x 480, two above); SSIM constants far from the defaults, where the kernel's short division must give
way to the full one; and the accumulator clear that rides on the loss kernels, where a second view follows a first with no K17 in between."""
import numpy as np
import pytest

from webdgs_amd import synth

import harness
import lossimages
from harness import assert_bits_equal
from test_gpu_dssim_loss import _lam, _loss_image, _pass

pytestmark = pytest.mark.gpu

LAMBDAS = [(0.8, 0.0, 0.2), (0.5, 0.3, 0.2), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]
# one pixel per thread (32 x 8 tiles): a single pixel; less than a window; exactly one tile, and one pixel more each way; a one-pixel-wide third tile
# column with a ragged last tile row; an ordinary odd size; and the largest that still takes this form
PPT1_SIZES = [(1, 1), (7, 5), (32, 8), (33, 9), (65, 43), (203, 117), (640, 480)]
# two pixels per thread (32 x 16 tiles): just past the switch, whole tiles vertically; a 9-row tail (a thread's pair straddles the last row) with a last
# tile column of 28; a last tile column of one pixel over a second tile row of one pixel, every window clamped vertically
PPT2_SIZES = [(641, 480), (700, 441), (19201, 17)]


def _assert_equals_oracle(got, want, what):
    """Bit for bit; where the oracle has a NaN the kernel must have one (any payload), and nowhere else."""
    gn, wn = np.isnan(got), np.isnan(want)
    apart = np.flatnonzero(gn != wn)
    assert apart.size == 0, f"{what}: the kernel has {int(gn.sum())} NaN, the oracle {int(wn.sum())}; first difference at flat index {int(apart[0])}"
    assert_bits_equal(np.where(wn, np.float32(0), got), np.where(wn, np.float32(0), want), what)


@pytest.mark.parametrize("w,h", PPT1_SIZES + PPT2_SIZES)
def test_loss_image_equals_the_oracle(hip_device, orc, w, h):
    dev = hip_device
    bwd = _pass(dev, w, h)
    try:
        for k, kind in enumerate(lossimages.KINDS):
            a, b = lossimages.pair(kind, w, h, seed=w * 7919 + h * 31 + k)
            ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
            for lam in LAMBDAS:
                bwd.setTrainingConfig(_lam(lam))
                got = _loss_image(bwd, ba, bb, w, h)
                assert np.all(got[..., 3] == 1.0), f"{w}x{h} {kind} {lam}: alpha lane"
                if kind == "identical":
                    assert np.all(got[..., :3] == 0.0), f"{w}x{h} {lam}: identical images must give exactly 0"
                assert_bits_equal(got, orc.loss_grad(a, b, orc.training_config(*lam)), f"loss image {w}x{h} {kind} {lam}")
    finally:
        bwd.destroy()


def _flat_windows(w=40, h=20):
    """Black against black with a patch of value 1 in b, and a band of 255 against 254: flat windows, whose SSIM denominator is about c1 * c2."""
    a, b = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)
    a[..., 3] = b[..., 3] = 255
    b[3:7, 5:11, :3] = 1
    a[12:17, :, :3], b[12:17, :, :3] = 255, 254
    return a, b


def test_ssim_constants_outside_the_defaults(hip_device, orc):
    """c1 = c2 from 1e-2 down to 1e-30, and a negative c1.  With c1 * c2 below the range the short division is verified on (test_gpu_math.py: 1e-8)
    the kernel has to divide in full: at 1e-20 the denominator of a black window is the subnormal 1e-40, whose reciprocal is not finite, and at 1e-30
    it is 0 and the quotient the oracle's NaN."""
    dev = hip_device
    w, h = 40, 20
    lam = (0.5, 0.3, 0.2)
    a, b = _flat_windows(w, h)
    ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
    bwd = _pass(dev, w, h, **_lam(lam))
    failures = []
    try:
        for c1, c2 in [(c, c) for c in (1e-2, 1e-6, 1e-12, 1e-17, 1e-20, 1e-30)] + [(-1e-4, 9e-4)]:
            bwd.setTrainingConfig(dict(c1=c1, c2=c2))
            got = _loss_image(bwd, ba, bb, w, h)
            want = orc.loss_grad(a, b, orc.training_config(*lam, c1, c2))
            assert np.isnan(want).any() == (c1 == 1e-30), f"c1 = {c1}: the oracle's NaNs are where c1 * c2 underflows to 0, and only there"
            assert np.all(got[..., 3] == 1.0)
            try:
                _assert_equals_oracle(got, want, f"loss image, c1 = {c1}, c2 = {c2}")
            except AssertionError as e:     # every constant is judged, and reported, before the test fails
                print(f"MISMATCH {e}")
                failures.append(str(e))
            else:
                print(f"c1 = {c1}, c2 = {c2}: equal to the oracle ({int(np.isnan(want).sum())} NaN)")
    finally:
        bwd.destroy()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("w,h", [(16, 16), (700, 441)])
@pytest.mark.parametrize("mode", ["reference", "gaussian"])
def test_a_second_raster_pass_clears_what_the_first_left(hip_device, orc, mode, w, h):
    """K15 + K16 of view A, then of view B, with no K17 in between: the clear that rides on B's loss kernel (lossimage.h: clear_dirty_accumulators, in
    loss_grad_kernel and dssim_grad_kernel alike) is all that removes A's sums from the Gaussians B does not touch.  At 16 x 16 the loss kernels'
    grids are one or two workgroups, which stride over all 60 000 quads; 700 x 441 is the two-pixels-per-thread grid."""
    dev = hip_device
    cfg = harness.small_config("c1", num_points=20000, width=w, height=h)
    n = cfg.num_points
    g, sh = synth.make_gaussians(cfg)
    # (view B chosen with the oracle's K1: of the 20 000 Gaussians the identity camera sees, it misses 13 469 at 16 x 16 and 1 277 at 700 x 441)
    cam_a, cam_b = synth.identity_camera(cfg), synth.circle_cameras(cfg, 8)[3]
    target = dev.bufferFrom(lossimages.pair("noise", w, h, seed=17)[0])
    tc = dict(dssim_mode=mode)

    def raster(pipe, cam):
        pipe.camera.write(cam)
        pipe.forward()
        pipe.bwd.encodeRaster(None, pipe.rast.getOutputTextureView(), target, pipe.backward_resources())
        dev.synchronize()
        return pipe.fwd.getResources()["tileCountsBuffer"].read(np.uint32)[:n], pipe.bwd.getAccumulatorsBuffer().read(np.int32)

    both = harness.HipPipeline(dev, cfg, g, sh, cam_a, training_config=tc)
    fresh = harness.HipPipeline(dev, cfg, g, sh, cam_b, training_config=tc)
    try:
        counts_a, acc_a = raster(both, cam_a)
        counts_b, acc_ab = raster(both, cam_b)
        only_a = (counts_a > 0) & (counts_b == 0)
        assert only_a.sum() >= 100, f"{int(only_a.sum())} Gaussians are visible in A and not in B"
        assert np.any(acc_a.reshape(-1, 12)[:n][only_a] != 0), "view A left nothing on the Gaussians that only it sees"
        _, acc_b = raster(fresh, cam_b)
        assert np.any(acc_b != 0)
        assert_bits_equal(acc_ab, acc_b, f"{mode} {w}x{h}: accumulators after views A, B vs after view B alone")
        # and view B alone is the oracle's backward raster of the GPU's own loss image
        fw = fresh.collect_forward()
        loss = fresh.bwd.getLossTextureView().read(np.float32).reshape(h, w, 4)
        bs = synth.render_settings(cfg).copy()
        bs[5] = 0.0
        gm, gc, go, gcol = orc.backward_rasterize(bs, n, fw["tile_ranges"], fw["sorted_values"], fw["splats"], fw["final_T"], fw["n_contrib"], loss)
        hm, hc, ho, hcol = harness.acc_to_reference_layout(acc_b, n)
        assert_bits_equal(hm, gm, "mean accumulators")
        assert_bits_equal(hc, gc, "conic accumulators")
        assert_bits_equal(ho, go, "opacity accumulators")
        assert_bits_equal(hcol, gcol, "colour accumulators")
    finally:
        both.destroy()
        fresh.destroy()
