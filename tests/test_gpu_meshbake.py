"""GPU: vertex colours baked from photographs (csrc/meshbake.hip).  Every byte of the sums, the view counts, the totals, the colours and
the mask equals the restatement (tests/meshbake_ref.py): the crafted cases -- every vertex count in all four kernel forms over the four image sizes, the
borders of the image, the guard band, the near plane, the depth rule and the weight rule at their edges, a camera block of another size -- several views in
two orders, recording, reuse at a larger and a smaller size, the refusals against sentinel-filled state, resolve's thresholds and fallbacks, the icosphere
under the zoo's cameras with the rasterizer's own depth images, and the Trainer surface."""
import hashlib

import numpy as np
import pytest

from webdgs_amd import _lib, ops

import harness
import meshbake_ref as B
import meshraster_ref as R
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


class _Uploaded:
    """A case on the device: vertices, normals, fallback, and per view camera, image and depth."""

    def __init__(self, dev, m):
        self.dev, self.m, self.V = dev, m, m["vertices"].shape[0]
        up = lambda a: None if a is None else dev.bufferFrom(np.ascontiguousarray(a))
        self.vertices, self.normals, self.fallback = up(m["vertices"]), up(m["normals"]), up(m["fallback"])
        self.views = [(up(w["camera"]), up(w["image"]), up(w["depth"])) for w in m["views"]]

    def accumulate(self, baker, k):
        w, (camera, image, depth) = self.m["views"][k], self.views[k]
        baker.accumulate(self.vertices, self.V, camera, image, w["width"], w["height"], self.normals, depth, w["near"], w["depth_tolerance"], w["min_cos"])

    def destroy(self):
        self.dev.synchronize()
        for b in [self.vertices, self.normals, self.fallback] + [x for v in self.views for x in v]:
            if b is not None:
                b.destroy()


def _resolve(dev, baker, V, fallback, min_views, min_weight, alias=None):
    """``(colours u8[V,4], baked u8[V])`` through sentinel-filled outputs with one word and four bytes of slack behind them.  ``alias``: the fallback
    colours as numpy, put into the output array, which is then its own fallback."""
    colours, mask = dev.createBuffer(4 * V + 4), dev.createBuffer(V + 4)
    try:
        colours.write(np.full(V + 1, SENTINEL, np.uint32))
        mask.write(np.full(V + 4, 0xA5, np.uint8))
        if alias is not None and V:
            colours.write(np.ascontiguousarray(alias, np.uint8))
        baker.resolve(colours, V, colours if alias is not None else fallback, mask, min_views, min_weight)
        c, k = colours.read(np.uint8), mask.read(np.uint8)
        assert np.all(c[4 * V:] == 0xA5) and np.all(k[V:V + 4] == 0xA5), "resolve wrote past the last vertex"
        return c[:4 * V].reshape(V, 4), k[:V]
    finally:
        colours.destroy()
        mask.destroy()


def _assert_state(baker, want, what, resolved=True):
    sums, views = baker.read()
    assert sums.dtype == np.uint64 and sums.shape == want["sums"].shape and views.dtype == np.uint32, f"{what}: the state is {sums.dtype}{sums.shape}"
    assert_bits_equal(sums, want["sums"], f"{what}: sums")
    assert_bits_equal(views, want["views"], f"{what}: views")
    assert baker.stats() == (want["totals"] if resolved else dict(want["totalsBeforeResolve"], bakedVertices=0)), f"{what}: {baker.stats()}"


def _assert_resolved(got, want, what):
    colours, mask = got
    assert_bits_equal(colours, want["colours"], f"{what}: colours")
    assert_bits_equal(mask, want["baked"].astype(np.uint8), f"{what}: mask")


# ---------------------------------------------------------------- 1. the crafted cases
@pytest.mark.parametrize("name", sorted(B.CASES))
def test_every_byte_equals_the_restatement(hip_device, name):
    dev = hip_device
    m, want = B.case(name), B.expected(name)
    up, baker = _Uploaded(dev, m), ops.MeshColourBaker(dev)
    try:
        baker.reset(up.V)
        for k in range(len(m["views"])):
            up.accumulate(baker, k)
        _assert_state(baker, want, name, resolved=False)
        _assert_resolved(_resolve(dev, baker, up.V, up.fallback, m["min_views"], m["min_weight"]), want, name)
        _assert_state(baker, want, f"{name}, after the resolve")
    finally:
        baker.destroy()
        up.destroy()


def test_three_views_in_two_orders_give_identical_bytes(hip_device):
    dev = hip_device
    m, want = B.case(B.THREE_VIEWS), B.expected(B.THREE_VIEWS)
    up, baker = _Uploaded(dev, m), ops.MeshColourBaker(dev)
    try:
        for order in ((0, 1, 2), (2, 0, 1)):
            baker.reset(up.V)
            for k in order:
                up.accumulate(baker, k)
            _assert_state(baker, want, f"order {order}", resolved=False)
            _assert_resolved(_resolve(dev, baker, up.V, up.fallback, m["min_views"], m["min_weight"]), want, f"order {order}")
    finally:
        baker.destroy()
        up.destroy()


# ---------------------------------------------------------------- 2. state: recording, reuse, refusals
def test_recorded_accumulate_and_resolve_replayed_twice_equal_two_eager_views(hip_device):
    dev = hip_device
    m = B.case("random-1000-67x45-depth")
    twice = B.run(m, order=(0, 0))
    up, recorded, eager = _Uploaded(dev, m), ops.MeshColourBaker(dev), ops.MeshColourBaker(dev)
    V = up.V
    colours, mask = dev.createBuffer(4 * V), dev.createBuffer(V)
    try:
        recorded.reset(V)
        eager.reset(V)
        with pytest.raises(_lib.StateError):   # a reset cannot be recorded
            with dev.createCommandEncoder("doomed", record=True):
                recorded.reset(V)
        dev.synchronize()
        with dev.createCommandEncoder("bake", record=True) as enc:
            up.accumulate(recorded, 0)
            recorded.resolve(colours, V, up.fallback, mask, m["min_views"], m["min_weight"])
            for waits in (recorded.stats, recorded.read):
                with pytest.raises(_lib.StateError):
                    waits()
            cmd = enc.finish()
        sums, views = recorded.read()
        assert not sums.any() and not views.any() and not any(recorded.stats().values()), "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
            up.accumulate(eager, 0)
        dev.synchronize()
        cmd.destroy()
        _assert_state(recorded, twice, "recorded once, replayed twice")
        _assert_resolved((colours.read(np.uint8).reshape(V, 4), mask.read(np.uint8)), twice, "the replayed resolve")
        _assert_state(eager, twice, "two eager views", resolved=False)
        assert np.all(twice["views"][twice["views"] > 0] == 2)
    finally:
        recorded.destroy()
        eager.destroy()
        up.destroy()
        colours.destroy()
        mask.destroy()


def test_one_object_takes_a_larger_then_a_smaller_mesh(hip_device):
    dev = hip_device
    baker = ops.MeshColourBaker(dev)
    try:
        for name in ("random-255-5x3", "random-1000-5x3-normals", "random-1-2x2", "random-0-1x1", "random-257-5x3-depth", "random-1000-5x3-normals"):
            m, want = B.case(name), B.expected(name)
            up = _Uploaded(dev, m)
            try:
                baker.reset(up.V)
                for k in range(len(m["views"])):
                    up.accumulate(baker, k)
                _assert_state(baker, want, f"reused object: {name}", resolved=False)
                _assert_resolved(_resolve(dev, baker, up.V, up.fallback, m["min_views"], m["min_weight"]), want, f"reused object: {name}")
            finally:
                up.destroy()
    finally:
        baker.destroy()
        baker.destroy()   # idempotent


def test_refusals_write_nothing(hip_device):
    dev = hip_device
    m, want = B.case("random-256-5x3-depth-normals"), B.expected("random-256-5x3-depth-normals")
    up, baker = _Uploaded(dev, m), ops.MeshColourBaker(dev)
    V, w = up.V, m["views"][0]
    camera, image, depth = up.views[0]
    colours, mask = dev.createBuffer(4 * V), dev.createBuffer(V)
    good = dict(vertices=up.vertices, numVertices=V, camera=camera, image=image, width=w["width"], height=w["height"], normals=up.normals, meshDepth=depth, near=w["near"],
                depthTolerance=w["depth_tolerance"], minCos=w["min_cos"])
    try:
        for early in (lambda: baker.accumulate(**good), lambda: baker.resolve(colours, V), baker.read, baker.stats):   # no reset precedes them
            with pytest.raises(_lib.StateError):
                early()
        with pytest.raises(_lib.WdgsError) as e:
            baker.reset(2 ** 31)
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.StateError):   # the refused reset left the object without a size
            baker.read()
        baker.reset(V)
        for k in range(len(m["views"])):
            up.accumulate(baker, k)
        _assert_state(baker, want, "before the refusals", resolved=False)
        colours.write(np.full(V, SENTINEL, np.uint32))
        mask.write(np.full(V, 0xA5, np.uint8))
        nan, inf = float("nan"), float("inf")
        invalid = (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf),
                   dict(depthTolerance=-1.0), dict(depthTolerance=nan), dict(depthTolerance=inf), dict(minCos=-0.25), dict(minCos=1.5), dict(minCos=nan),
                   dict(camera=None), dict(image=None), dict(vertices=None),
                   # (a misaligned buffer is refused before anything is read: the view's size is never used)
                   dict(vertices=dev.view(up.vertices.ptr + 2, up.vertices.size)), dict(normals=dev.view(up.normals.ptr + 1, up.normals.size)),
                   dict(camera=dev.view(camera.ptr + 2, camera.size)), dict(image=dev.view(image.ptr + 3, image.size)), dict(meshDepth=dev.view(depth.ptr + 2, depth.size)))
        for kw in invalid:
            with pytest.raises(_lib.WdgsError) as e:
                baker.accumulate(**dict(good, **kw))
            assert e.value.code == _lib.WDGS_E_INVALID, kw
        for kw in (dict(numVertices=V - 1), dict(numVertices=V // 2), dict(numVertices=0)):   # another V than the reset's
            with pytest.raises(_lib.StateError):
                baker.accumulate(**dict(good, **kw))
        with pytest.raises(ValueError):   # (more vertices than the buffers hold never reach the library)
            baker.accumulate(**dict(good, numVertices=V + 1))
        with pytest.raises(ValueError):
            baker.accumulate(**dict(good, image=dev.view(image.ptr, image.size - 4)))
        with pytest.raises(_lib.StateError):
            baker.resolve(colours, V - 1, up.fallback, mask)
        for bad in ((None, V, up.fallback, mask), (dev.view(colours.ptr + 2, colours.size), V, up.fallback, mask), (colours, V, dev.view(up.fallback.ptr + 1, 4 * V), mask)):
            with pytest.raises(_lib.WdgsError) as e:
                baker.resolve(*bad)
            assert e.value.code == _lib.WDGS_E_INVALID
        dev.synchronize()
        assert np.all(colours.read(np.uint32) == SENTINEL) and np.all(mask.read(np.uint8) == 0xA5), "a refused call wrote an output"
        _assert_state(baker, want, "after the refusals", resolved=False)
        # a camera block of another image size: the call is taken and accumulates nothing
        other = dev.bufferFrom(R.crafted_camera(w["width"], w["height"], block_size=(w["width"] + 1, w["height"])))
        try:
            baker.accumulate(**dict(good, camera=other))
            mismatched = dict(want, totalsBeforeResolve=dict(want["totalsBeforeResolve"], viewportMismatch=1))
            _assert_state(baker, mismatched, "after a mismatched view", resolved=False)
        finally:
            other.destroy()
    finally:
        baker.destroy()
        up.destroy()
        colours.destroy()
        mask.destroy()


# ---------------------------------------------------------------- 3. resolve
def test_resolve_thresholds_and_fallbacks(hip_device):
    dev = hip_device
    m = B.case(B.THREE_VIEWS)
    ref = B.new_state(m["vertices"].shape[0])
    for w in m["views"]:
        B.accumulate(ref, m["vertices"], m["normals"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"])
    sums, views = B.arrays(ref)
    two = int(np.flatnonzero(views == 2)[0])
    at_views, at_weight = 2, int(sums[two, 3])
    assert np.any(views == 1) and np.any(views == 3) and 1 < at_weight
    up, baker = _Uploaded(dev, m), ops.MeshColourBaker(dev)
    try:
        baker.reset(up.V)
        for k in range(3):
            up.accumulate(baker, k)
        rules = [(0, 0), (1, 1), (at_views, 1), (at_views + 1, 1), (1, at_weight), (1, at_weight + 1), (4, 1), (1, 2 ** 40), (2 ** 32 - 1, 2 ** 64 - 1)]
        for min_views, min_weight in rules:   # each threshold at equality and one past (vertex `two`)
            for what, fallback, alias in (("fallback", up.fallback, None), ("no fallback", None, None), ("fallback aliased onto the output", up.fallback, m["fallback"])):
                colours, baked = B.resolve(ref, m["fallback"] if fallback is not None else None, min_views, min_weight)
                got = _resolve(dev, baker, up.V, fallback, min_views, min_weight, alias)
                _assert_resolved(got, dict(colours=colours, baked=baked), f"min_views {min_views}, min_weight {min_weight}, {what}")
                assert baker.stats()["bakedVertices"] == int(baked.sum())
                if fallback is None:
                    assert not got[0][~baked].any(), "no fallback: zeros"
        for (min_views, min_weight), is_baked in (((at_views, 1), 1), ((at_views + 1, 1), 0), ((1, at_weight), 1), ((1, at_weight + 1), 0)):
            assert _resolve(dev, baker, up.V, None, min_views, min_weight)[1][two] == is_baked
        for bad in (dict(minViews=-1), dict(minViews=2 ** 32), dict(minWeight=2 ** 64)):
            with pytest.raises(_lib.WdgsError):
                baker.resolve(None, up.V, **bad)
    finally:
        baker.destroy()
        up.destroy()


# ---------------------------------------------------------------- 4. end to end: the icosphere under the zoo's cameras, the rasterizer's own depth
def _sphere_reference(tolerance, min_cos, occlusion, images, normals=True):
    """The restatement over the three cameras, fed by ``meshraster_ref``'s depth images."""
    first = B.sphere(B.SPHERE_CAMERAS[0])
    state = B.new_state(first["vertices"].shape[0])
    for name, image in zip(B.SPHERE_CAMERAS, images):
        s = B.sphere(name)
        depth = R.rasterize(first["vertices"], first["faces"], None, s["camera"], s["width"], s["height"], s["near"])["depth"] if occlusion else None
        B.accumulate(state, first["vertices"], first["normals"] if normals else None, s["camera"], image, depth, s["width"], s["height"], s["near"], tolerance, min_cos)
    return state


def test_the_icosphere_under_rolled_steep_and_close_cameras(hip_device):
    dev = hip_device
    spheres = [B.sphere(name) for name in B.SPHERE_CAMERAS]
    s0 = spheres[0]
    V, w, h = s0["vertices"].shape[0], s0["width"], s0["height"]
    assert V == 162 and all(s["width"] == w and s["height"] == h for s in spheres)
    # (the roll37 and below spheres are one mesh; the close camera looks at it from further off than at its own)
    mesh = dict(vertices=s0["vertices"], faces=s0["faces"], colours=s0["colours"], normals=s0["normals"])
    cameras, images = [s["camera"] for s in spheres], [s["image"] for s in spheres]
    tolerance, min_cos = 0.0625, 0.1
    results = {}
    for occlusion in (True, False):
        ref = _sphere_reference(tolerance, min_cos, occlusion, images)
        before = dict(ref["totals"])
        colours, baked = B.resolve(ref, s0["colours"])
        got = ops.bakeVertexColours(dev, mesh, cameras, images, w, h, depthTolerance=tolerance, minCos=min_cos, near=s0["near"], occlusion=occlusion)
        assert_bits_equal(got["colours"], colours[:, :3], f"occlusion={occlusion}: colours")
        assert got["colours"].shape == (V, 3) and got["baked"].dtype == bool
        assert np.array_equal(got["baked"], baked), f"occlusion={occlusion}: mask"
        assert got["stats"] == dict(before, bakedVertices=int(baked.sum())), got["stats"]
        assert np.array_equal(got["colours"][~baked], s0["colours"][~baked][:, :3]), "an unbaked vertex keeps its fallback"
        results[occlusion] = got
    with_, without = results[True]["baked"], results[False]["baked"]
    assert np.all(without[with_]), "a vertex baked with occlusion is baked without it"
    assert 0 < with_.sum() < without.sum(), "occlusion takes the silhouettes' vertices out"
    # a constant photograph gives exactly that colour; the state through MeshColourBaker, with the normals computed on the device
    flat = [np.broadcast_to(np.array([9, 200, 31, 0], np.uint8), (h, w, 4)).copy() for _ in spheres]
    got = ops.bakeVertexColours(dev, dict(vertices=s0["vertices"], faces=s0["faces"]), cameras, flat, w, h, depthTolerance=tolerance, near=s0["near"])
    assert got["baked"].any() and np.all(got["colours"][got["baked"]] == np.array([9, 200, 31], np.uint8)) and not got["colours"][~got["baked"]].any()
    with pytest.raises(ValueError):
        ops.bakeVertexColours(dev, mesh, cameras, images[:2], w, h)
    # on the device, left there
    src = dict(vertices=dev.bufferFrom(s0["vertices"]), faces=dev.bufferFrom(s0["faces"]), colours=dev.bufferFrom(s0["colours"]), normals=dev.bufferFrom(s0["normals"]),
               numVertices=V, numFaces=s0["faces"].shape[0])
    out = {}
    try:
        out = ops.bakeVertexColours(dev, src, [dev.bufferFrom(c) for c in cameras], [dev.bufferFrom(i) for i in images], w, h, depthTolerance=tolerance, minCos=min_cos,
                                    near=s0["near"], asBuffers=True)
        rgba = out["colours"].read(np.uint8, count=4 * V).reshape(V, 4)
        assert_bits_equal(rgba[:, :3], results[True]["colours"], "asBuffers: colours")
        assert np.array_equal(rgba[:, 3] == 255, results[True]["baked"] | (s0["colours"][:, 3] == 255))
        assert np.array_equal(out["baked"].read(np.uint8, count=V).astype(bool), results[True]["baked"])
    finally:
        ops.destroyBuffers({k: v for k, v in out.items() if isinstance(v, ops.HipBuffer) and k in ("colours", "baked")})
        ops.destroyBuffers({k: v for k, v in src.items() if isinstance(v, ops.HipBuffer)})


# ---------------------------------------------------------------- 5. the Trainer surface
def _state_digest(t):
    t.flushPointCloud()
    hsh = hashlib.sha256()
    hsh.update(t.pointCloud.gaussian_3d_buffer.read(np.uint32).tobytes())
    hsh.update(t.pointCloud.sh_buffer.read(np.uint32).tobytes())
    return hsh.hexdigest(), t.iteration, t._rng.getstate()


def test_trainer_bakes_and_extract_mesh_takes_the_option(hip_device):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t, never = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False), _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    keys = ("vertices", "faces", "colours", "keys")
    try:
        for trainer in (t, never):
            for _ in range(4):
                trainer.step()
            trainer.drain()
        t.fuseDepth(vol)
        parent = ops.weldTriangles(vol.extractTriangles(1.0))   # what extractMesh returned before it took the option
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == set(keys)
        for what, mesh in (("without the option", raw), ("bake=None spelled out", t.extractMesh(lo, hi, voxel, bake=None))):
            for k in keys:
                assert_bits_equal(mesh[k], parent[k], f"extractMesh {what}: {k}")
        V = raw["vertices"].shape[0]
        before = _state_digest(t)
        # bakeMeshColours = ops.bakeVertexColours over the trainer's own cameras and photographs
        baked = t.bakeMeshColours(raw, depthTolerance=voxel)
        photographs = [im["texture"].read(np.uint8).reshape(cfg.height, cfg.width, 4) for im in imgs]
        want = ops.bakeVertexColours(dev, raw, [c["camera"] for c in cameras], photographs, cfg.width, cfg.height, depthTolerance=voxel)
        assert baked["views"] == [0, 1, 2, 3] and baked["stats"] == want["stats"] and 0 < baked["stats"]["bakedVertices"] < V
        assert_bits_equal(baked["colours"], want["colours"], "bakeMeshColours: colours")
        assert np.array_equal(baked["baked"], want["baked"]) and baked["colours"].shape == (V, 3)
        assert np.array_equal(baked["colours"][~baked["baked"]], raw["colours"][~baked["baked"]]), "an unbaked vertex keeps the fused colour"
        assert np.any(baked["colours"][baked["baked"]] != raw["colours"][baked["baked"]]), "the photographs' colours are not the fused ones"
        one = t.bakeMeshColours(raw, viewIds=[2], depthTolerance=voxel)
        assert one["views"] == [2] and 0 < one["stats"]["bakedVertices"] <= baked["stats"]["bakedVertices"] and np.all(baked["baked"][one["baked"]])
        with pytest.raises(TypeError):
            t.bakeMeshColours(raw, depthTolerence=voxel)
        # extractMesh(bake=...) bakes last, on the final mesh
        got = t.extractMesh(lo, hi, voxel, bake=dict(depthTolerance=voxel))
        for k in ("vertices", "faces", "keys"):
            assert_bits_equal(got[k], raw[k], f"extractMesh(bake): {k}")
        assert_bits_equal(got["colours"], baked["colours"], "extractMesh(bake): colours")
        assert got["bakeStats"] == baked["stats"] and "normals" not in got and "stats" not in got
        for weld in ("host", "device"):
            base = t.extractMesh(lo, hi, voxel, weld=weld, minTriangles=20, smooth=2, simplify=2 * voxel, normals=True)
            got = t.extractMesh(lo, hi, voxel, weld=weld, minTriangles=20, smooth=2, simplify=2 * voxel, normals=True, bake=True)
            for k in ("vertices", "faces", "normals"):
                assert_bits_equal(got[k], base[k], f"extractMesh(simplify, bake), weld={weld}: {k}")
            want = t.bakeMeshColours(base)
            assert_bits_equal(got["colours"], want["colours"], f"extractMesh(simplify, bake), weld={weld}: colours")
            assert got["stats"] == base["stats"] and got["bakeStats"] == want["stats"] and got["bakeStats"]["bakedVertices"] > 0
        reference = np.random.default_rng(4).uniform(lo, hi, (3000, 3)).astype(np.float32)
        r = t.evaluateGeometry(reference, lo, hi, voxel, maxDistance=8.0, threshold=0.5, bake=True)
        assert r["vertices"] == V and np.isfinite(r["chamfer"])
        assert _state_digest(t) == before, "training state is untouched"
        for trainer in (t, never):
            trainer.step()
            trainer.drain()
        assert _state_digest(t) == _state_digest(never), "the next step's bytes are those of a trainer that never baked"
    finally:
        vol.destroy()
        t.destroy()
        never.destroy()
