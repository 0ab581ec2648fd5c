"""GPU: per-face visibility over views, the rule on its counters and the face filter on the device (csrc/meshvisibility.hip).  Every
byte equals the restatement (tests/meshvisibility_ref.py): the crafted face images -- no faces, one pixel, nothing but empty pixels, one face on an odd and on a
large image, two faces alternating, runs of every length from 1 to 130, random faces among few and among many, foreign indices -- the depth rule at its edges,
several views, recording, reuse, the refusals, the rule's four thresholds, the filter against ``removeSmallComponents`` and under crafted masks, the icosphere
under the zoo's cameras end to end, and the Trainer surface."""
import hashlib

import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshclean_ref as M
import meshraster_ref as R
import meshvisibility_ref as VR
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
MESH_KEYS = ("vertices", "faces", "vertexMap", "faceMap")


def _depths(n, seed):
    """Mesh depth, model depth and weight sum for n pixels: close pairs, with absent, non-finite and negative values mixed in."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 5.0, n).astype(np.float32)
    b = (a + rng.uniform(-0.1, 0.1, n).astype(np.float32)).astype(np.float32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    kind = rng.integers(0, 12, n)
    for k, (arr, value) in enumerate(((a, 0.0), (b, 0.0), (b, np.nan), (b, np.inf), (b, -1.0), (a, np.inf))):
        arr[kind == k] = value
    return a, b, w


def _accumulate(dev, vis, img, w, h, depths=None, min_weight_sum=0.5, threshold=0.05):
    """One eager accumulate of numpy images; the uploads are released once the stream has run."""
    bufs = [dev.bufferFrom(np.ascontiguousarray(img, np.uint32))] + [None if x is None else dev.bufferFrom(np.ascontiguousarray(x, np.float32)) for x in (depths or ())]
    try:
        vis.accumulate(bufs[0], w, h, *bufs[1:], minWeightSum=min_weight_sum, threshold=threshold)
        dev.synchronize()
    finally:
        for b in bufs:
            if b is not None:
                b.destroy()


def _assert_state(vis, ref, what):
    got = vis.read()
    assert got.dtype == np.uint32 and got.shape == ref.counters.shape, f"{what}: counters are {got.dtype}{got.shape}"
    assert_bits_equal(got, ref.counters, f"{what}: counters")
    assert vis.stats() == ref.stats(), f"{what}: {vis.stats()}"


# ---------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("name", sorted(VR.IMAGES))
def test_counters_equal_the_restatement(hip_device, name):
    dev = hip_device
    F, w, h, img = VR.image(name)
    a, b, ws = _depths(img.size, 3)
    vis = ops.FaceVisibility(dev)
    try:
        for what, depths in (("no depth", None), ("depth and weight sum", (a, b, ws)), ("depth", (a, b, None))):
            ref = VR.Accumulator(F)
            vis.reset(F)
            ref.accumulate(img, *(depths or ()), min_weight_sum=0.5, threshold=0.05)
            _accumulate(dev, vis, img, w, h, depths)
            _assert_state(vis, ref, f"{name}, {what}")
        if name == "no-faces":
            assert vis.buffer() is None and vis.stats()["foreignPixels"] == 48
    finally:
        vis.destroy()


def test_the_depth_rule_at_its_edges(hip_device):
    dev = hip_device
    t = np.float32(0.0625)   # (a power of two, so that 2 + t and the ulp above it are f32 values whose differences from 2 are exact)
    over = np.nextafter(np.float32(2.0) + t, np.float32(np.inf))
    below = np.nextafter(np.float32(0.5), np.float32(0))
    #                 model depth 0, nan, inf, < 0 | |a - b| = t, one ulp over | mesh depth absent | weight sum below, at | fine | not counted
    a = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0], np.float32)
    b = np.array([0.0, np.nan, np.inf, -1.0, np.float32(2.0) + t, over, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0], np.float32)
    ws = np.array([1, 1, 1, 1, 1, 1, 1, below, 0.5, 1, 1, 1], np.float32)
    img = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, VR.EMPTY, 77], np.uint32)
    assert np.float32(b[4] - a[4]) == t and np.float32(b[5] - a[5]) > t
    vis = ops.FaceVisibility(dev)
    try:
        for w, h in ((12, 1), (3, 4)):
            ref = VR.Accumulator(10)
            vis.reset(10)
            ref.accumulate(img, a, b, ws, 0.5, t)
            _accumulate(dev, vis, img, w, h, (a, b, ws), 0.5, float(t))
            _assert_state(vis, ref, f"depth edges {w}x{h}")
            assert vis.read()[:, 1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1, 1]
        vis.reset(10)
        _accumulate(dev, vis, img, 12, 1, (a, b, None), 0.5, float(t))
        assert vis.read()[:, 1].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 1]   # without the weight sum pixel 7 agrees
        vis.reset(10)
        _accumulate(dev, vis, img, 12, 1)
        assert vis.read().tolist() == [[1, 1, 1]] * 10 and vis.stats()["foreignPixels"] == 1   # the null-depth form
    finally:
        vis.destroy()


def test_views_over_three_different_images(hip_device):
    dev = hip_device
    F, w, h = 40, 53, 31
    rng = np.random.default_rng(7)
    images = [rng.integers(1, F, w * h).astype(np.uint32) for _ in range(3)]
    for k, img in enumerate(images):
        img[rng.integers(0, w * h, 200)] = VR.EMPTY
        if k != 1:
            img[rng.integers(0, w * h, 50)] = 0   # face 0: calls 1 and 3 only
        img[img == 5] = 6                         # face 5: one pixel per call
        img[100 * (k + 1)] = 5
    assert not np.any(images[1] == 0)
    vis, ref = ops.FaceVisibility(dev), VR.Accumulator(F)
    try:
        vis.reset(F)
        for k, img in enumerate(images):
            depths = _depths(w * h, 10 + k)
            ref.accumulate(img, *depths, min_weight_sum=0.25, threshold=0.07)
            _accumulate(dev, vis, img, w, h, depths, 0.25, 0.07)
            _assert_state(vis, ref, f"after view {k + 1}")
        got = vis.read()
        assert got[0, 2] == 2 and got[5].tolist()[::2] == [3, 3] and np.all(got[:, 2] <= 3) and vis.stats()["views"] == 3
    finally:
        vis.destroy()


# ---------------------------------------------------------------- 2. state: recording, repeats, reuse, refusals
def test_recorded_accumulate_replayed_twice_equals_two_eager_calls(hip_device):
    dev = hip_device
    F, w, h, img = VR.image("run-lengths")
    a, b, ws = _depths(img.size, 9)
    bufs = [dev.bufferFrom(x) for x in (img, a, b, ws)]
    recorded, eager = ops.FaceVisibility(dev), ops.FaceVisibility(dev)
    try:
        recorded.reset(F)
        eager.reset(F)
        with dev.createCommandEncoder("face visibility", record=True) as enc:
            recorded.accumulate(bufs[0], w, h, bufs[1], bufs[2], bufs[3], 0.5, 0.05)
            with pytest.raises(_lib.StateError):   # the statistics wait
                recorded.stats()
            cmd = enc.finish()
        assert not recorded.read().any() and recorded.stats()["views"] == 0, "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
            eager.accumulate(bufs[0], w, h, bufs[1], bufs[2], bufs[3], 0.5, 0.05)
        dev.synchronize()
        cmd.destroy()
        ref = VR.Accumulator(F)
        for _ in range(2):
            ref.accumulate(img, a, b, ws, 0.5, 0.05)
        _assert_state(eager, ref, "two eager calls")
        _assert_state(recorded, ref, "recorded once, replayed twice")
        assert np.all(ref.counters[ref.counters[:, 0] > 0, 2] == 2)
    finally:
        recorded.destroy()
        eager.destroy()
        for x in bufs:
            x.destroy()


def test_two_runs_agree_and_one_object_takes_larger_then_smaller_meshes(hip_device):
    dev = hip_device
    vis = ops.FaceVisibility(dev)
    try:
        first = None
        for name in ("random-5", "random-100000", "random-5", "one-pixel", "no-faces", "foreign", "random-100000"):   # a larger, then a smaller F on one object
            F, w, h, img = VR.image(name)
            ref = VR.Accumulator(F)
            vis.reset(F)
            for _ in range(2):
                ref.accumulate(img)
                _accumulate(dev, vis, img, w, h)
            _assert_state(vis, ref, f"reused object: {name}")
            if name == "random-100000":
                if first is None:
                    first = vis.read()
                else:
                    assert_bits_equal(vis.read(), first, "a second run")
    finally:
        vis.destroy()
        vis.destroy()   # idempotent


def test_refusals_write_nothing(hip_device):
    dev = hip_device
    F, w, h, img = VR.image("foreign")
    a, b, ws = _depths(img.size, 4)
    image, da, db, dw = (dev.bufferFrom(x) for x in (img, a, b, ws))
    vis, ref = ops.FaceVisibility(dev), VR.Accumulator(F)
    try:
        with pytest.raises(_lib.StateError):   # no reset precedes them
            vis.accumulate(image, w, h)
        with pytest.raises(_lib.StateError):
            vis.stats()
        with pytest.raises(_lib.StateError):
            vis.buffer()
        with pytest.raises(_lib.WdgsError):
            vis.reset(2 ** 31)
        vis.reset(F)
        ref.accumulate(img, a, b, ws, 0.5, 0.05)
        vis.accumulate(image, w, h, da, db, dw, 0.5, 0.05)
        counters = vis.buffer()
        before = counters.read(np.uint32)
        assert_bits_equal(before.reshape(F, 3), ref.counters, "before the refusals")
        counters.write(np.full(3 * F, SENTINEL, np.uint32))
        bad = (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")),
               dict(threshold=float("inf")), dict(meshDepth=None), dict(modelDepth=None), dict(meshDepth=None, modelDepth=None), dict(faceImage=None),
               # (a misaligned image is refused before anything is read: the view's size is never used)
               dict(faceImage=dev.view(image.ptr + 4, image.size)), dict(meshDepth=dev.view(da.ptr + 8, da.size)), dict(modelWeightSum=dev.view(dw.ptr + 4, dw.size)))
        for kw in bad:   # exactly one depth pointer null, a weight sum without depths, bad sizes and thresholds, null and misaligned images
            args = dict(dict(faceImage=image, width=w, height=h, meshDepth=da, modelDepth=db, modelWeightSum=dw, minWeightSum=0.5, threshold=0.05), **kw)
            with pytest.raises(_lib.WdgsError) as e:
                vis.accumulate(**args)
            assert e.value.code == _lib.WDGS_E_INVALID, kw
        with pytest.raises(ValueError):
            vis.accumulate(dev.view(image.ptr, image.size - 4), w, h)
        dev.synchronize()
        assert np.all(counters.read(np.uint32) == SENTINEL), "a refused call wrote the counters"
        assert vis.stats() == ref.stats()
        assert_bits_equal(vis.read(), ref.counters, "after the refusals")   # (read packs them anew)
        # a reset that has to grow the arrays cannot be recorded; one that does not can
        with pytest.raises(_lib.StateError):
            with dev.createCommandEncoder("doomed", record=True):
                vis.reset(F + 1000)
        dev.synchronize()
        assert vis.stats() == ref.stats()
    finally:
        vis.destroy()
        for x in (image, da, db, dw):
            x.destroy()


def test_overflow_is_refused_by_host_arithmetic(hip_device):
    """(views + 1) W H >= 2^32 is refused: 8192 x 8192 = 2^26 pixels as view 64, after 63 views of one pixel.  The refusal comes before the face image is
    looked at, so a null image serves and nothing large is allocated."""
    dev = hip_device
    pixel = dev.bufferFrom(np.array([1, SENTINEL, SENTINEL, SENTINEL], np.uint32))
    vis, ref = ops.FaceVisibility(dev), VR.Accumulator(2)
    try:
        vis.reset(2)
        with pytest.raises(_lib.WdgsError) as e:   # view 1 of that size is legal: the null image is what is refused
            vis.accumulate(None, 8192, 8192)
        assert e.value.code == _lib.WDGS_E_INVALID
        for k in range(63):
            if k == 62:
                assert not ref.would_overflow(8192, 8192)
                with pytest.raises(_lib.WdgsError) as e:   # view 63: 63 2^26 < 2^32
                    vis.accumulate(None, 8192, 8192)
                assert e.value.code == _lib.WDGS_E_INVALID and not isinstance(e.value, _lib.CapacityError)
            vis.accumulate(pixel, 1, 1)
            ref.accumulate(np.array([1], np.uint32))
        assert ref.would_overflow(8192, 8192) and not ref.would_overflow(8192, 8191)
        counters = vis.buffer()
        counters.write(np.full(6, SENTINEL, np.uint32))
        with pytest.raises(_lib.CapacityError):
            vis.accumulate(None, 8192, 8192)
        with pytest.raises(_lib.WdgsError) as e:   # one row less fits: refused for its null image only
            vis.accumulate(None, 8192, 8191)
        assert e.value.code == _lib.WDGS_E_INVALID
        dev.synchronize()
        assert np.all(counters.read(np.uint32) == SENTINEL), "a refused call wrote the counters"
        vis.accumulate(pixel, 1, 1)   # a small view is still taken
        ref.accumulate(np.array([1], np.uint32))
        _assert_state(vis, ref, "after the refusal")
        assert vis.read().tolist() == [[0, 0, 0], [64, 64, 64]]
        vis.reset(2)   # ... and a reset starts the count anew
        with pytest.raises(_lib.WdgsError) as e:
            vis.accumulate(None, 8192, 8192)
        assert e.value.code == _lib.WDGS_E_INVALID
    finally:
        vis.destroy()
        pixel.destroy()


# ---------------------------------------------------------------- 3. the rule
def test_flags_equal_the_restatement(hip_device):
    dev = hip_device
    rng = np.random.default_rng(41)
    pixels = rng.integers(0, 50, 5000)
    counters = np.stack([pixels, rng.integers(0, 51, 5000) * pixels // 50, rng.integers(0, 5, 5000)], axis=1).astype(np.uint32)
    counters[:8] = [[10, 5, 2], [10, 4, 2], [0, 0, 0], [3, 1, 1], [65536, 21845, 1], [65536, 21846, 1], [2 ** 32 - 1, 2 ** 32 - 1, 7], [2 ** 32 - 1, 2 ** 32 - 2, 1]]
    F = counters.shape[0]
    cbuf, keep = dev.bufferFrom(counters), dev.createBuffer(F + 4)
    rules = [dict(), dict(minPixels=0, minViews=0)]
    for name, at in (("minPixels", 10), ("minViews", 2), ("minAgreeing", 5)):   # each threshold alone, at and one past equality (face 0)
        rules += [dict(dict(minPixels=0, minViews=0), **{name: at}), dict(dict(minPixels=0, minViews=0), **{name: at + 1})]
    rules += [dict(minPixels=0, minViews=0, minAgreeingFraction=f) for f in (0.5, np.nextafter(0.5, 1.0) + 2.0 ** -17, 1.0 / 3.0, 21846 / 65536, 1.0, 0.0)]
    try:
        for rule in rules:
            keep.write(np.full(F + 4, 0xA5, np.uint8))
            ops.encodeFaceVisibilityFlags(dev, cbuf, F, keep, **rule)
            got = keep.read(np.uint8)
            want = VR.flags(counters, rule.get("minPixels", 1), rule.get("minViews", 1), rule.get("minAgreeing", 0), VR.fraction_q16(rule.get("minAgreeingFraction", 0.0)))
            assert_bits_equal(got[:F], want, f"flags {rule}")
            assert np.all(got[F:] == 0xA5), "flags past the last face"
            assert np.array_equal(ops.selectFaces(counters, **rule), want.astype(bool)), rule
        at, past = (keep_of[0] for keep_of in (VR.flags(counters, 0, 0, 0, 32768), VR.flags(counters, 0, 0, 0, 32769)))
        assert (at, past) == (1, 0) and VR.flags(counters, 0, 0, 0, 65536)[2] == 1 and VR.flags(counters, 1, 0, 0, 0)[2] == 0   # pixels = 0
        for bad in (dict(minAgreeingFraction=1.5), dict(minPixels=2 ** 32), dict(minViews=-1)):
            with pytest.raises(_lib.WdgsError):
                ops.encodeFaceVisibilityFlags(dev, cbuf, F, keep, **bad)
        with pytest.raises(_lib.WdgsError):
            ops.encodeFaceVisibilityFlags(dev, cbuf, 2 ** 31, keep)
        ops.encodeFaceVisibilityFlags(dev, None, 0, None)   # no faces: nothing to do
        with dev.createCommandEncoder("flags", record=True) as enc:   # it waits for nothing and records
            ops.encodeFaceVisibilityFlags(dev, cbuf, F, keep, minPixels=7)
            cmd = enc.finish()
        keep.clear()
        dev.queue.submit([cmd])
        dev.synchronize()
        cmd.destroy()
        assert_bits_equal(keep.read(np.uint8)[:F], VR.flags(counters, 7, 1, 0, 0), "recorded flags")
    finally:
        cbuf.destroy()
        keep.destroy()


# ---------------------------------------------------------------- 4. the filter
def _assert_mesh(got, want, what, keys=MESH_KEYS):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, f"{what}: {k}"
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} is {got[k].dtype}{got[k].shape}, not {want[k].dtype}{want[k].shape}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


def _cluster_mesh():
    faces, V, _ = M.shape("clusters")
    return dict(M.as_mesh(faces, V), colours=np.random.default_rng(2).integers(0, 256, (V, 3)).astype(np.uint8), keys=np.arange(V, dtype=np.uint64) * np.uint64(3))


@pytest.mark.parametrize("name", ["clusters", "only-invalid", "no-faces", "no-vertices", "one-face", "singletons"])
def test_all_ones_equals_remove_small_components_with_defaults(hip_device, name):
    dev = hip_device
    faces, V, labels = M.shape(name)
    mesh = M.as_mesh(faces, V)
    got, want = ops.filterFaces(dev, mesh, np.ones(faces.shape[0], bool)), ops.removeSmallComponents(dev, mesh)
    _assert_mesh(got, want, f"all ones: {name}")
    _assert_mesh(got, VR.filter_faces(mesh, np.ones(faces.shape[0], np.uint8)), f"all ones vs the restatement: {name}")
    assert got["invalidFaces"] == labels["invalidFaces"]


def test_masks_colours_keys_and_buffers(hip_device):
    dev = hip_device
    mesh = _cluster_mesh()
    faces, V = mesh["faces"], mesh["vertices"].shape[0]
    F = faces.shape[0]
    valid = np.all(faces.astype(np.int64) < V, axis=1)
    masks = {"all zeros": np.zeros(F, np.uint8), "alternate faces": (np.arange(F) % 2 == 0).astype(np.uint8) * 255, "only invalid faces": (~valid).astype(np.uint8),
             "random": (np.random.default_rng(3).integers(0, 4, F) == 0).astype(np.uint8)}
    for what, keep in masks.items():
        got, want = ops.filterFaces(dev, mesh, keep), VR.filter_faces(mesh, keep)
        _assert_mesh(got, want, what, MESH_KEYS + ("colours", "keys"))   # colours and keys follow vertexMap
        assert got["invalidFaces"] == want["invalidFaces"] == int((~valid).sum())
    for what in ("all zeros", "only invalid faces"):
        got = ops.filterFaces(dev, mesh, masks[what])
        assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["keys"].shape == (0,)
    with pytest.raises(ValueError):
        ops.filterFaces(dev, mesh, np.ones(F - 1, bool))
    # a mesh and a mask on the device, and the result left there
    want = VR.filter_faces(mesh, masks["random"])
    src = dict(vertices=dev.bufferFrom(mesh["vertices"]), faces=dev.bufferFrom(mesh["faces"]), numVertices=V, numFaces=F)
    kbuf = dev.bufferFrom(masks["random"])
    out = {}
    try:
        out = ops.filterFaces(dev, src, kbuf, asBuffers=True)
        kv, kf = out["numVertices"], out["numFaces"]
        assert (kv, kf) == (want["vertices"].shape[0], want["faces"].shape[0]) and "colours" not in out
        got = dict(vertices=out["vertices"].read(np.float32, count=3 * kv).reshape(kv, 3), faces=out["faces"].read(np.uint32, count=3 * kf).reshape(kf, 3),
                   vertexMap=out["vertexMap"].read(np.uint32, count=kv), faceMap=out["faceMap"].read(np.uint32, count=kf))
        _assert_mesh(got, want, "asBuffers")
        assert_bits_equal(src["faces"].read(np.uint32).reshape(F, 3), faces, "the input is left as it is")
    finally:
        ops.destroyBuffers({k: v for k, v in out.items() if isinstance(v, ops.HipBuffer)})
        ops.destroyBuffers(dict(src, keep=kbuf))


def test_filter_capacity_state_and_recording(hip_device):
    dev = hip_device
    mesh = _cluster_mesh()
    faces, V = mesh["faces"], mesh["vertices"].shape[0]
    F = faces.shape[0]
    keep = (np.random.default_rng(8).integers(0, 3, F) != 0).astype(np.uint8)
    want = VR.filter_faces(mesh, keep)
    kv, kf = want["vertices"].shape[0], want["faces"].shape[0]
    vbuf, fbuf, kbuf = dev.bufferFrom(mesh["vertices"]), dev.bufferFrom(faces), dev.bufferFrom(keep)
    outs = [dev.createBuffer(n) for n in (12 * kv, 12 * kf, 4 * kv, 4 * kf)]
    filt = ops.MeshFaceFilter(dev)
    try:
        with pytest.raises(_lib.StateError):   # no select precedes it
            filt.compact(vbuf, *outs)
        for bad in ((None, 3, 10, kbuf), (fbuf, 3, 10, None), (fbuf, 2 ** 31, 10, kbuf), (fbuf, 10, 2 ** 31, kbuf)):
            with pytest.raises(_lib.WdgsError) as e:
                filt.select(*bad)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.StateError):   # the selection waits for its counts
            with dev.createCommandEncoder("doomed", record=True):
                filt.select(fbuf, F, V, kbuf)
        dev.synchronize()
        assert filt.select(fbuf, F, V, kbuf) == (kv, kf, want["invalidFaces"])
        for b in outs:
            b.write(np.full(b.size // 4, SENTINEL, np.uint32))
        for cv, cf in ((kv - 1, kf), (kv, kf - 1), (0, 0)):   # one short on either array
            with pytest.raises(_lib.CapacityError):
                filt.compact(vbuf, *outs, capacityVertices=cv, capacityFaces=cf)
        dev.synchronize()
        for b in outs:
            assert np.all(b.read(np.uint32) == SENTINEL), "a refused compaction wrote something"
        with dev.createCommandEncoder("compact", record=True) as enc:   # the compaction waits for nothing and records
            filt.compact(vbuf, *outs)
            cmd = enc.finish()
        assert np.all(outs[1].read(np.uint32) == SENTINEL), "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
            dev.synchronize()
            got = dict(vertices=outs[0].read(np.float32).reshape(kv, 3), faces=outs[1].read(np.uint32).reshape(kf, 3), vertexMap=outs[2].read(np.uint32),
                       faceMap=outs[3].read(np.uint32))
            _assert_mesh(got, want, "recorded compact, replayed")
            outs[1].clear()
        cmd.destroy()
        filt.compact(None, None, outs[1])   # without positions and maps
        assert_bits_equal(outs[1].read(np.uint32).reshape(kf, 3), want["faces"], "compact without positions: faces")
        assert filt.select(fbuf, 0, V, None) == (0, 0, 0) and filt.select(None, 0, 0, None) == (0, 0, 0)
    finally:
        filt.destroy()
        filt.destroy()   # idempotent
        for b in outs + [vbuf, fbuf, kbuf]:
            b.destroy()


# ---------------------------------------------------------------- 5. end to end: the icosphere under the zoo's cameras
def test_removing_what_no_view_saw_changes_no_pixel(hip_device):
    dev = hip_device
    m = R.case("sphere-roll37")
    mesh = dict(vertices=m["vertices"], faces=m["faces"], colours=m["colours"])
    w, h, F = m["width"], m["height"], m["faces"].shape[0]
    assert m["vertices"].shape[0] == 162
    cameras = [R.case(name)["camera"] for name in ("sphere-roll37", "sphere-below", "sphere-close")]   # rolled, steep, close
    assert all(R.case(name)["width"] == w and R.case(name)["height"] == h for name in ("sphere-below", "sphere-close"))
    full = [R.expected("sphere-roll37"), R.expected("sphere-below"), R.rasterize(m["vertices"], m["faces"], None, cameras[2], w, h, m["near"])]
    ref = VR.Accumulator(F)
    for r in full:
        ref.accumulate(r["face"])
    got = ops.faceVisibility(dev, mesh, cameras, w, h, m["near"])
    assert_bits_equal(got["counters"], ref.counters, "faceVisibility vs the restatement fed by meshraster_ref's face images")
    assert got["stats"] == ref.stats() and got["stats"]["foreignPixels"] == 0 and got["stats"]["countedPixels"] > 1000
    assert np.array_equal(got["counters"][:, 1], got["counters"][:, 0])
    keep = ops.selectFaces(got["counters"])
    assert 0 < keep.sum() < F, "some faces, and not all, are seen"
    culled = ops.filterFaces(dev, mesh, keep)
    assert culled["faces"].shape[0] == int(keep.sum()) and culled["vertices"].shape[0] < 162
    _assert_mesh(culled, VR.filter_faces(mesh, keep), "the culled sphere", MESH_KEYS + ("colours",))
    new_index = np.full(F + 1, R.NO_FACE, np.uint32)
    new_index[culled["faceMap"]] = np.arange(culled["faceMap"].size, dtype=np.uint32)
    for camera, r in zip(cameras, full):
        mine = ops.rasterizeMesh(dev, culled, camera, w, h, m["near"])
        assert_bits_equal(mine["depth"], r["depth"], "the culled mesh's depth image")
        assert_bits_equal(culled["faceMap"][np.minimum(mine["face"], culled["faceMap"].size - 1)][mine["face"] != R.NO_FACE], r["face"][r["face"] != R.NO_FACE],
                          "the culled mesh's face image through faceMap")
        assert_bits_equal(mine["face"], new_index[np.minimum(r["face"], F)], "the full mesh's face image through the inverse of faceMap")
    # a stricter rule removes more, and then pixels do change
    fewer = ops.selectFaces(got["counters"], minViews=2)
    assert fewer.sum() < keep.sum()


# ---------------------------------------------------------------- 6. the Trainer surface
def _state_digest(t):
    t.flushPointCloud()
    hsh = hashlib.sha256()
    hsh.update(t.pointCloud.gaussian_3d_buffer.read(np.uint32).tobytes())
    hsh.update(t.pointCloud.sh_buffer.read(np.uint32).tobytes())
    return hsh.hexdigest(), t.iteration, t._rng.getstate()


def test_trainer_cull_mesh_and_extract_mesh_take_the_rule(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    try:
        for _ in range(4):
            t.step()
        t.drain()
        t.fuseDepth(vol)
        parent = ops.weldTriangles(vol.extractTriangles(1.0))   # what extractMesh returned before it took the option
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == {"vertices", "faces", "colours", "keys"}
        _assert_mesh(raw, parent, "extractMesh without the option", ("vertices", "faces", "colours", "keys"))
        _assert_mesh(t.extractMesh(lo, hi, voxel, cull=None), parent, "cull=None spelled out", ("vertices", "faces", "colours", "keys"))
        F = raw["faces"].shape[0]
        before = _state_digest(t)
        # meshVisibility
        vis = t.meshVisibility(raw, threshold=voxel)
        c = vis["counters"]
        assert c.shape == (F, 3) and vis["views"] == [0, 1, 2, 3] and vis["iteration"] == t.iteration
        assert int(c[:, 0].astype(np.int64).sum()) == sum(vis["counted"]) and int(c[:, 1].astype(np.int64).sum()) == sum(vis["agreeing"]) and vis["foreign"] == [0] * 4
        assert np.all(c[:, 1] <= c[:, 0]) and np.all(c[:, 2] <= 4) and np.array_equal(c[:, 2] > 0, c[:, 0] > 0)
        assert all(0 < n <= cfg.width * cfg.height for n in vis["counted"]) and sum(vis["agreeing"]) > 0
        one = t.meshVisibility(raw, viewIds=[2], threshold=voxel)
        assert (one["counted"], one["agreeing"]) == ([vis["counted"][2]], [vis["agreeing"][2]]) and np.all(one["counters"][:, 2] <= 1)
        on_device = dict(vertices=dev.bufferFrom(raw["vertices"]), faces=dev.bufferFrom(raw["faces"]), numVertices=raw["vertices"].shape[0], numFaces=F)
        try:
            assert_bits_equal(t.meshVisibility(on_device, threshold=voxel)["counters"], c, "a mesh on the device")
        finally:
            ops.destroyBuffers(on_device)
        # cullMesh = meshVisibility + selectFaces + filterFaces by hand
        for rule in (dict(), dict(minViews=2), dict(minPixels=4, minAgreeingFraction=0.5), dict(minAgreeing=1)):
            keep = ops.selectFaces(c, **rule)
            assert 0 < keep.sum() < F, f"{rule}: the fused mesh has faces no view sees"
            got, want = t.cullMesh(raw, threshold=voxel, **rule), ops.filterFaces(dev, raw, keep)
            _assert_mesh(got, want, f"cullMesh {rule}", MESH_KEYS + ("colours", "keys"))
            assert_bits_equal(got["counters"], c, f"cullMesh {rule}: counters")
            assert got["views"] == [0, 1, 2, 3]
        with pytest.raises(TypeError):
            t.cullMesh(raw, treshold=voxel)
        # extractMesh(cull=...) = cullMesh(extractMesh()) and then the later stages, with both welds
        rule = dict(minPixels=2, threshold=voxel)
        for weld in ("host", "device"):
            base = t.extractMesh(lo, hi, voxel, weld=weld, minTriangles=20)
            culled = t.cullMesh(base, **rule)
            got = t.extractMesh(lo, hi, voxel, weld=weld, minTriangles=20, cull=rule)
            _assert_mesh(got, culled, f"extractMesh(cull), weld={weld}", MESH_KEYS + ("colours", "keys"))
            assert got["faces"].shape[0] < base["faces"].shape[0]
            got = t.extractMesh(lo, hi, voxel, weld=weld, minTriangles=20, cull=rule, smooth=3, normals=True)
            want = ops.smoothMesh(dev, culled, 3)
            _assert_mesh(got, want, f"extractMesh(cull, smooth), weld={weld}", ("vertices", "faces"))
            assert_bits_equal(got["normals"], ops.vertexNormals(dev, want), f"extractMesh(cull, smooth, normals), weld={weld}")
            assert got["stats"]["boundaryEdges"] > 0, "smoothing sees the boundary the cut made"
        simplified = t.extractMesh(lo, hi, voxel, cull=dict(threshold=voxel), simplify=2 * voxel)
        want = ops.simplifyMesh(dev, t.cullMesh(raw, threshold=voxel), 2 * voxel, np.asarray(lo, np.float32))
        _assert_mesh(simplified, want, "extractMesh(cull, simplify)", ("vertices", "faces", "colours"))
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        r = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, cull=dict(threshold=voxel))
        assert r["faces"] == int(ops.selectFaces(c).sum()) and all(np.isfinite(r[k]) for k in ("accuracy", "completeness", "chamfer"))
        assert _state_digest(t) == before, "training state is untouched"
    finally:
        vol.destroy()
        t.destroy()
