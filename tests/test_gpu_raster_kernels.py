"""GPU: rasterize (K14) and backward_rasterize (K16) driven directly on the crafted tile lists of tests/rastercases.py -- no projection, no sort.
K14 runs through the test hook wdgs_debug_rasterize, in both of its bodies (nf_stamp NULL: EXACT; stamps that match nowhere: fast; and, on grids of
several tiles, stamps on every other tile); K16 through TiledBackwardPass.encodeRaster on the case's tables, the ORACLE's final T and n_contrib and
a crafted image pair with lambda = (0, lambda_l2, 0).  Every comparison is bit for bit against the parity oracle on the same arrays: rgba8, final T,
n_contrib; the loss image; the four accumulator arrays, the rows of unlisted Gaussians (zero), and blue's four partial sums word by word.  What makes
the oracle right at these corners is tests/test_raster_cases.py (float64)."""
import ctypes as C

import numpy as np
import pytest

from webdgs_amd import _lib, ops

import rastercases as rc
from harness import acc_to_reference_layout, assert_bits_equal

pytestmark = pytest.mark.gpu

GUARD = 16                     # sentinel elements behind every image the hook writes
SENTINEL = 0xDEADBEEF
_oracle = {}


def oracle_forward(orc, case):
    if case["name"] not in _oracle:
        rows = np.ascontiguousarray(case["rows"][:case["num_splats"]])
        _oracle[case["name"]] = orc.rasterize(rc.settings_array(case), rc.tile_info_array(case), rows, case["ranges"], case["keys"], case["vals"], case["count"],
                                              case["max_batches"])
    return _oracle[case["name"]]


def _buf(dev, a):
    a = np.ascontiguousarray(a)
    return dev.bufferFrom(a if a.size else np.zeros(1, a.dtype))


class Tables:
    """A case's tables on the device, and the three images the hook writes (with guard words behind them)."""

    def __init__(self, dev, case):
        self.dev, self.case = dev, case
        self.px = case["W"] * case["H"]
        self.T = int(case["ranges"].size - 1)
        self.splats, self.keys, self.vals, self.ranges = (_buf(dev, case[k]) for k in ("rows", "keys", "vals", "ranges"))
        self.count = _buf(dev, np.array([case["count"]], np.uint32))
        self.frame_word = _buf(dev, np.array([1], np.uint32))
        self.images = [dev.createBuffer(4 * (self.px + GUARD)) for _ in range(3)]

    def frame(self, stamps, **over):
        c = self.case
        f = dict(viewport_width=c["W"], viewport_height=c["H"], max_splat_radius_px=c["cap"], point_size_px=c["point"], render_mode=c["mode"],
                 num_splats=c["num_splats"], max_batches=c["max_batches"], splats=self.splats.ptr, sorted_keys=self.keys.ptr, sorted_vals=self.vals.ptr,
                 count=self.count.ptr, ranges=self.ranges.ptr, nf_stamp=stamps.ptr if stamps is not None else None,
                 nf_frame=self.frame_word.ptr if stamps is not None else None)
        f.update(over)
        return _lib.DebugRasterFrame(**f)

    def call(self, frame, images="own"):
        ptrs = [b.ptr for b in self.images] if images == "own" else images
        return self.dev.lib.wdgs_debug_rasterize(self.dev.handle, C.byref(frame) if frame is not None else None, *ptrs)

    def rasterize(self, body):
        """body: "exact" (no stamps), "fast" (stamps that match the frame word nowhere) or "mixed" (every other tile stamped)."""
        stamps = None
        if body != "exact":
            st = np.zeros(self.T, np.uint32)
            if body == "mixed":
                st[::2] = 1
            stamps = _buf(self.dev, st)
        for b in self.images:
            b.write(np.full(self.px + GUARD, SENTINEL, np.uint32))
        _lib.check(self.call(self.frame(stamps)))
        c = self.case
        out = [b.read(np.uint32) for b in self.images]
        for o, what in zip(out, ("rgba8", "final T", "n_contrib")):
            assert_bits_equal(o[self.px:], np.full(GUARD, SENTINEL, np.uint32), f"{c['name']} ({body}): the words behind the {what} image")
        self.dev.synchronize()
        return (out[0][:self.px].view(np.uint8).reshape(c["H"], c["W"], 4), out[1][:self.px].view(np.float32).reshape(c["H"], c["W"]),
                out[2][:self.px].reshape(c["H"], c["W"]))


def _same_forward(got, ref, what):
    for g, r, name in zip(got, ref, ("rgba8", "final T", "n_contrib")):
        assert_bits_equal(g, r, f"{what}: {name}")


class Backward:
    """A TiledBackwardPass sized to a case; run() = encodeRaster on the case's tables with the given final T / n_contrib buffers."""

    def __init__(self, dev, case, tables):
        self.dev, self.case, self.t = dev, case, tables
        self.N = int(case["rows"].shape[0])
        pc = ops.PointCloud("full", self.N, 0, None, None)
        self.op = ops.TiledBackwardPass(dev, pc, dict(viewportWidth=case["W"], viewportHeight=case["H"], maxSplatRadiusPx=case["cap"] if case["cap"] != 0.0 else 128.0,
                                                      trainingConfig=dict(lambda_l1=0.0, lambda_l2=case["lam"], lambda_dssim=0.0)))
        self.pred, self.targ = _buf(dev, case["pred"]), _buf(dev, case["targ"])

    def run(self, final_T, n_contrib, targ=None):
        res = dict(splatBuffer=self.t.splats, tileOffsetsBuffer=self.t.ranges, tileIndicesBuffer=self.t.vals, alphaTexture=final_T, nContribTexture=n_contrib)
        self.op.encodeRaster(None, self.pred, targ if targ is not None else self.targ, res)
        c = self.case
        loss = self.op.getLossTextureView().read(np.float32).reshape(c["H"], c["W"], 4)
        acc = self.op.getAccumulatorsBuffer().read(np.int32).reshape(-1, 12)[:self.N]
        self.dev.synchronize()
        return loss, acc

    def destroy(self):
        self.op.destroy()


def _oracle_backward(orc, case, T, ncon, loss):
    return orc.backward_rasterize(rc.settings_array(case, backward=True), case["rows"].shape[0], case["ranges"], case["vals"], case["rows"],
                                  np.ascontiguousarray(T), np.ascontiguousarray(ncon), np.ascontiguousarray(loss))


def _check_backward(orc, case, loss, acc, T, ncon, what):
    tcfg = orc.training_config(0.0, case["lam"], 0.0)
    assert_bits_equal(loss, orc.loss_grad(case["pred"], case["targ"], tcfg), f"{what}: loss image")
    want = _oracle_backward(orc, case, T, ncon, loss)
    for g, w, name in zip(acc_to_reference_layout(acc, acc.shape[0]), want, ("means", "conics", "opacity", "colours")):
        assert_bits_equal(g, w, f"{what}: accumulated {name}")
    unlisted = np.setdiff1d(np.arange(acc.shape[0]), case["vals"])
    assert not acc[unlisted].any(), f"{what}: rows of Gaussians that are in no list"


def _blue_partials(orc, case, T, ncon, loss):
    """Words 8..11 of every accumulator row as the oracle gives them: blue summed over the pixel rows 2r, 2r + 1 of every 8x8 block (one 16-lane row
    of the producing wave) for r = 0..3 -- integer sums are additive over pixels, so four runs on masked loss images give them exactly."""
    y = np.arange(case["H"])[:, None, None]
    return np.stack([_oracle_backward(orc, case, T, ncon, np.where((y % 8) // 2 == r, loss, np.float32(0.0)).astype(np.float32))[3].reshape(-1, 3)[:, 2] for r in range(4)], 1)


@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6, 7, 8])
def test_rasterize_equals_the_oracle_in_both_bodies(hip_device, orc, fam):
    cases = rc.family(fam)
    assert cases
    for case in cases:
        t = Tables(hip_device, case)
        ref = oracle_forward(orc, case)
        for body in ("exact", "fast") + (("mixed",) if t.T > 1 else ()):
            _same_forward(t.rasterize(body), ref, f"{case['name']} ({body} body)")


@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6, 7, 8])
def test_backward_rasterize_equals_the_oracle(hip_device, orc, fam):
    cases = [c for c in rc.family(fam) if c["k16"]]
    assert cases
    for case in cases:
        t = Tables(hip_device, case)
        _, T, ncon = oracle_forward(orc, case)
        b = Backward(hip_device, case, t)
        try:
            loss, acc = b.run(_buf(hip_device, T), _buf(hip_device, ncon))
            _check_backward(orc, case, loss, acc, T, ncon, case["name"])
            if fam == 7:
                assert_bits_equal(acc[:, 8:12], _blue_partials(orc, case, T, ncon, loss), f"{case['name']}: blue's four partial sums (words 8..11)")
        finally:
            b.destroy()


CHAINED = ("chunk table", "saturation staircase", "full chunks then the next tile", "block cull at the 1/255 contour", "9 tiles", "values beyond num_splats")


def test_backward_rasterize_on_the_hooks_own_outputs(hip_device, orc):
    """K14's images handed to K16 as device buffers, never through the host: the same bits as from the oracle's images."""
    for name in CHAINED:
        case = next(c for c in rc.all_cases() if c["name"] == name)
        t = Tables(hip_device, case)
        got = t.rasterize("fast")
        _same_forward(got, oracle_forward(orc, case), name)
        b = Backward(hip_device, case, t)
        try:
            view = lambda buf: hip_device.view(buf.ptr, 4 * t.px)
            loss, acc = b.run(view(t.images[1]), view(t.images[2]))
            _check_backward(orc, case, loss, acc, got[1], got[2], name + " (chained)")
        finally:
            b.destroy()


def test_argument_checks(hip_device, orc):
    """What a forward pass can never hand the kernel is refused with WDGS_E_INVALID and the hook's name; a valid call afterwards still works."""
    case = next(c for c in rc.all_cases() if c["name"] == "9 tiles")
    t = Tables(hip_device, case)
    own = [b.ptr for b in t.images]
    stamps = _buf(hip_device, np.zeros(t.T, np.uint32))
    refused = [("null device", lambda: hip_device.lib.wdgs_debug_rasterize(None, C.byref(t.frame(None)), *own)),
               ("null frame", lambda: t.call(None)),
               ("null rgba8", lambda: t.call(t.frame(None), [None, own[1], own[2]])), ("null final T", lambda: t.call(t.frame(None), [own[0], None, own[2]])),
               ("null n_contrib", lambda: t.call(t.frame(None), [own[0], own[1], None])),
               ("zero width", lambda: t.call(t.frame(None, viewport_width=0))), ("zero height", lambda: t.call(t.frame(None, viewport_height=0))),
               ("65535 tiles", lambda: t.call(t.frame(None, viewport_width=16 * 65535, viewport_height=16))),
               ("4096 x 4096 px", lambda: t.call(t.frame(None, viewport_width=4096, viewport_height=4096))),
               ("stamps without a frame word", lambda: t.call(t.frame(stamps, nf_frame=None)))]
    refused += [(f"null {k}", (lambda k=k: t.call(t.frame(None, **{k: None})))) for k in ("splats", "sorted_keys", "sorted_vals", "count", "ranges")]
    for what, call in refused:
        code = call()
        assert code == _lib.WDGS_E_INVALID, f"{what}: returned {code}"
        with pytest.raises(_lib.WdgsError) as err:
            _lib.check(code)
        assert err.value.code == _lib.WDGS_E_INVALID and "wdgs_debug_rasterize" in str(err.value), what
    _same_forward(t.rasterize("mixed"), oracle_forward(orc, case), "a valid call after the refusals")
