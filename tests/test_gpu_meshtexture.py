"""GPU: a texture atlas baked from photographs (csrc/meshtexture.hip).  Every byte of the rows, the texture, the texel states and the
totals equals the restatement (tests/meshtexture_ref.py): the crafted cases -- every face count at every cell size, the wave's tail at C = 4, cells of several
waves, every face-level and texel-level rule, the image's edge, a camera block of another size, resolve's fill, thresholds and fallbacks -- several views in two
orders, recording, reuse at a larger and a smaller size, the refusals against sentinel-filled state, the refusal of the 65536th view, the icosphere under the
zoo's cameras with the rasterizer's own depth images, the analytic ramp, which does not go through the restatement, and the Trainer surface with the OBJ it ends in."""
import numpy as np
import pytest

from webdgs_amd import _lib, loaders, ops

import harness
import meshraster_ref as R
import meshtexture_ref as T
from harness import assert_bits_equal
from test_gpu_eval import _trainer, _views

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


class _Uploaded:
    """A case on the device: vertices, faces, colours, and per view camera, image and depth."""

    def __init__(self, dev, m):
        self.dev, self.m, self.V, self.F = dev, m, m["vertices"].shape[0], m["faces"].shape[0]
        up = lambda a: None if a is None or a.size == 0 else dev.bufferFrom(np.ascontiguousarray(a))
        self.vertices, self.faces, self.colours = up(m["vertices"]), up(m["faces"]), up(m["colours"])
        self.views = [(up(w["camera"]), up(w["image"]), up(w["depth"])) for w in m["views"]]

    def accumulate(self, baker, k):
        w, (camera, image, depth) = self.m["views"][k], self.views[k]
        baker.accumulate(self.vertices, self.V, self.faces, self.F, camera, image, w["width"], w["height"], depth, w["near"], w["depth_tolerance"], w["min_cos"],
                         w["two_sided"])

    def destroy(self):
        self.dev.synchronize()
        for b in [self.vertices, self.faces, self.colours] + [x for v in self.views for x in v]:
            if b is not None:
                b.destroy()


def _resolve(dev, baker, up, min_weight, fill, colours="own"):
    """``(texture u8[Ht,Wt,4], texelState u8[Ht,Wt])`` through sentinel-filled outputs with one word and four bytes of slack behind them."""
    n = baker.width * baker.height
    texture, state = dev.createBuffer(4 * n + 4), dev.createBuffer(n + 4)
    try:
        texture.write(np.full(n + 1, SENTINEL, np.uint32))
        state.write(np.full(n + 4, 0xA5, np.uint8))
        baker.resolve(up.faces, up.F, up.V, texture, up.colours if colours == "own" else colours, state, min_weight, fill)
        t, s = texture.read(np.uint8), state.read(np.uint8)
        assert np.all(t[4 * n:] == 0xA5) and np.all(s[n:n + 4] == 0xA5), "resolve wrote past the last texel"
        return t[:4 * n].reshape(baker.height, baker.width, 4), s[:n].reshape(baker.height, baker.width)
    finally:
        texture.destroy()
        state.destroy()


def _assert_state(baker, want, what, resolved=True):
    rows = baker.read()
    assert rows.dtype == np.uint32 and rows.shape == want["rows"].shape, f"{what}: the state is {rows.dtype}{rows.shape}"
    assert_bits_equal(rows, want["rows"], f"{what}: rows")
    totals = want["totals"] if resolved else dict(want["totals"], bakedTexels=0, filledTexels=0, fallbackTexels=0)
    assert baker.stats() == totals, f"{what}: {baker.stats()} != {totals}"


def _assert_resolved(got, want, what):
    assert_bits_equal(got[0], want["texture"], f"{what}: texture")
    assert_bits_equal(got[1], want["texelState"], f"{what}: texel states")


def _bake(dev, baker, name, what=None):
    m, want = T.case(name), T.expected(name)
    up = _Uploaded(dev, m)
    try:
        L = baker.reset(up.F, m["cell"])
        ref = T.layout(up.F, m["cell"])
        assert L == dict(width=ref["width"], height=ref["height"], cellsPerRow=ref["cellsPerRow"])
        for k in range(len(m["views"])):
            up.accumulate(baker, k)
        _assert_state(baker, want, what or name, resolved=False)
        _assert_resolved(_resolve(dev, baker, up, m["min_weight"], m["fill"]), want, what or name)
        _assert_state(baker, want, f"{what or name}, after the resolve")
    finally:
        up.destroy()


# ---------------------------------------------------------------- 1. the crafted cases
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_every_byte_equals_the_restatement(hip_device, name):
    baker = ops.MeshTextureBaker(hip_device)
    try:
        _bake(hip_device, baker, name)
    finally:
        baker.destroy()


def test_three_views_in_two_orders_give_identical_bytes(hip_device):
    dev = hip_device
    m, want = T.case(T.THREE_VIEWS), T.expected(T.THREE_VIEWS)
    up, baker = _Uploaded(dev, m), ops.MeshTextureBaker(dev)
    try:
        for order in ((0, 1, 2), (2, 0, 1)):
            baker.reset(up.F, m["cell"])
            for k in order:
                up.accumulate(baker, k)
            _assert_state(baker, want, f"order {order}", resolved=False)
            _assert_resolved(_resolve(dev, baker, up, m["min_weight"], m["fill"]), want, f"order {order}")
    finally:
        baker.destroy()
        up.destroy()


def test_resolve_without_fill_and_without_colours(hip_device):
    dev = hip_device
    m = T.case("resolve-colours")
    up, baker = _Uploaded(dev, m), ops.MeshTextureBaker(dev)
    try:
        baker.reset(up.F, m["cell"])
        ref = T.new_state(up.F, m["cell"])
        for k, w in enumerate(m["views"]):
            up.accumulate(baker, k)
            T.accumulate(ref, m["vertices"], m["faces"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"],
                         w["two_sided"])
        top = int(ref["rows"][:, 3].max())
        for min_weight in (0, 1, top, top + 1, 2 ** 32 - 1):   # the threshold at equality and one past
            for fill in (True, False):
                for colours in ("own", None):
                    texture, state = T.resolve(ref, m["faces"], m["colours"] if colours == "own" else None, up.V, min_weight, fill)
                    what = f"min_weight {min_weight}, fill {fill}, colours {colours}"
                    _assert_resolved(_resolve(dev, baker, up, min_weight, fill, colours), dict(texture=texture, texelState=state), what)
                    s = baker.stats()
                    assert (s["bakedTexels"], s["filledTexels"], s["fallbackTexels"]) == tuple(ref["totals"][k] for k in ("bakedTexels", "filledTexels", "fallbackTexels")), what
                    assert fill or s["filledTexels"] == 0
            assert (T.resolve(ref, m["faces"], None, up.V, top, False)[1] == 1).sum() >= 1 and not (T.resolve(ref, m["faces"], None, up.V, top + 1, False)[1] == 1).any()
    finally:
        baker.destroy()
        up.destroy()


# ---------------------------------------------------------------- 2. state: recording, reuse, refusals
def test_recorded_accumulate_and_resolve_replayed_twice_equal_two_eager_views(hip_device):
    dev = hip_device
    m = T.case("faces-129-cell-8")
    twice = T.run(m, order=(1, 1))
    up, recorded, eager = _Uploaded(dev, m), ops.MeshTextureBaker(dev), ops.MeshTextureBaker(dev)
    L = recorded.reset(up.F, m["cell"])
    n = L["width"] * L["height"]
    texture, state = dev.createBuffer(4 * n), dev.createBuffer(n)
    try:
        eager.reset(up.F, m["cell"])
        with pytest.raises(_lib.StateError):   # a reset cannot be recorded
            with dev.createCommandEncoder("doomed", record=True):
                recorded.reset(up.F, m["cell"])
        dev.synchronize()
        with dev.createCommandEncoder("bake", record=True) as enc:
            up.accumulate(recorded, 1)
            recorded.resolve(up.faces, up.F, up.V, texture, up.colours, state, m["min_weight"], m["fill"])
            for waits in (recorded.stats, recorded.read):
                with pytest.raises(_lib.StateError):
                    waits()
            cmd = enc.finish()
        assert not recorded.read().any() and not any(recorded.stats().values()), "recording runs nothing"
        for _ in range(2):
            dev.queue.submit([cmd])
            up.accumulate(eager, 1)
        dev.synchronize()
        cmd.destroy()
        _assert_state(recorded, twice, "recorded once, replayed twice")
        _assert_resolved((texture.read(np.uint8).reshape(L["height"], L["width"], 4), state.read(np.uint8).reshape(L["height"], L["width"])), twice, "the replayed resolve")
        _assert_state(eager, twice, "two eager views", resolved=False)
    finally:
        recorded.destroy()
        eager.destroy()
        up.destroy()
        texture.destroy()
        state.destroy()


def test_one_object_takes_a_larger_then_a_smaller_mesh(hip_device):
    baker = ops.MeshTextureBaker(hip_device)
    try:
        for name in ("faces-7-cell-8", "faces-129-cell-16", "faces-1-cell-4", "faces-0-cell-8", "faces-11-cell-32", "faces-129-cell-4", "faces-129-cell-16"):
            _bake(hip_device, baker, name, f"reused object: {name}")
    finally:
        baker.destroy()
        baker.destroy()   # idempotent


def test_refusals_write_nothing(hip_device):
    dev = hip_device
    name = "faces-11-cell-8"
    m, want = T.case(name), T.expected(name)
    up, baker = _Uploaded(dev, m), ops.MeshTextureBaker(dev)
    V, F, w = up.V, up.F, m["views"][1]
    camera, image, depth = up.views[1]
    L = T.layout(F, m["cell"])
    n = L["width"] * L["height"]
    texture, state = dev.createBuffer(4 * n), dev.createBuffer(n)
    good = dict(vertices=up.vertices, numVertices=V, faces=up.faces, numFaces=F, camera=camera, image=image, width=w["width"], height=w["height"], meshDepth=depth,
                near=w["near"], depthTolerance=w["depth_tolerance"], minCos=w["min_cos"])
    try:
        for early in (lambda: baker.accumulate(**good), lambda: baker.resolve(up.faces, F, V, texture), baker.read, baker.stats, baker.layout):   # no reset precedes them
            with pytest.raises(_lib.StateError):
                early()
        for bad in ((2 ** 31, 8), (F, 0), (F, 5), (F, 64), (2 * (16384 // 8) ** 2 + 1, 8), (2 * (16384 // 32) ** 2 + 1, 32)):
            with pytest.raises(_lib.WdgsError) as e:
                baker.reset(*bad)
            assert e.value.code == _lib.WDGS_E_INVALID, bad
        with pytest.raises(_lib.WdgsError) as e:
            baker.reset(F, 8, _accumulates=65536)
        assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(_lib.StateError):   # the refused resets left the object without a size
            baker.read()
        baker.reset(F, m["cell"])
        for k in range(len(m["views"])):
            up.accumulate(baker, k)
        _assert_state(baker, want, "before the refusals", resolved=False)
        texture.write(np.full(n, SENTINEL, np.uint32))
        state.write(np.full(n, 0xA5, np.uint8))
        nan, inf = float("nan"), float("inf")
        invalid = (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf),
                   dict(depthTolerance=-1.0), dict(depthTolerance=nan), dict(depthTolerance=inf), dict(minCos=-0.25), dict(minCos=1.5), dict(minCos=nan),
                   dict(camera=None), dict(image=None), dict(vertices=None), dict(faces=None), dict(numVertices=2 ** 31),
                   # (a misaligned buffer is refused before anything is read: the view's size is never used)
                   dict(vertices=dev.view(up.vertices.ptr + 2, up.vertices.size)), dict(faces=dev.view(up.faces.ptr + 1, up.faces.size)),
                   dict(camera=dev.view(camera.ptr + 2, camera.size)), dict(image=dev.view(image.ptr + 3, image.size)), dict(meshDepth=dev.view(depth.ptr + 2, depth.size)))
        for kw in invalid:
            with pytest.raises(_lib.WdgsError) as e:
                baker.accumulate(**dict(good, **kw))
            assert e.value.code == _lib.WDGS_E_INVALID, kw
        for kw in (dict(numFaces=F - 1), dict(numFaces=F // 2), dict(numFaces=0)):   # another F than the reset's
            with pytest.raises(_lib.StateError):
                baker.accumulate(**dict(good, **kw))
        with pytest.raises(ValueError):   # (more faces than the buffer holds never reach the library)
            baker.accumulate(**dict(good, numFaces=F + 1))
        with pytest.raises(ValueError):
            baker.accumulate(**dict(good, image=dev.view(image.ptr, image.size - 4)))
        with pytest.raises(_lib.StateError):
            baker.resolve(up.faces, F - 1, V, texture, up.colours, state)
        for bad in ((up.faces, F, V, None), (None, F, V, texture), (up.faces, F, V, dev.view(texture.ptr + 2, texture.size)), (dev.view(up.faces.ptr + 2, up.faces.size), F, V, texture),
                    (up.faces, F, V, texture, dev.view(up.colours.ptr + 1, up.colours.size))):
            with pytest.raises(_lib.WdgsError) as e:
                baker.resolve(*bad)
            assert e.value.code == _lib.WDGS_E_INVALID
        with pytest.raises(ValueError):
            baker.resolve(up.faces, F, V, dev.view(texture.ptr, texture.size - 4))
        dev.synchronize()
        assert np.all(texture.read(np.uint32) == SENTINEL) and np.all(state.read(np.uint8) == 0xA5), "a refused call wrote an output"
        _assert_state(baker, want, "after the refusals", resolved=False)
        # a camera block of another image size: the call is taken and accumulates nothing
        other = dev.bufferFrom(R.crafted_camera(w["width"], w["height"], block_size=(w["width"] + 1, w["height"])))
        try:
            baker.accumulate(**dict(good, camera=other))
            _assert_state(baker, dict(want, totals=dict(want["totals"], viewportMismatch=1)), "after a mismatched view", resolved=False)
        finally:
            other.destroy()
    finally:
        baker.destroy()
        up.destroy()
        texture.destroy()
        state.destroy()


def test_the_65536th_view_is_refused(hip_device):
    dev = hip_device
    m = T.case("faces-3-cell-8")
    up, baker = _Uploaded(dev, m), ops.MeshTextureBaker(dev)
    try:
        baker.reset(up.F, m["cell"], _accumulates=65534)
        up.accumulate(baker, 0)   # the 65535th
        one = T.new_state(up.F, m["cell"])
        w = m["views"][0]
        T.accumulate(one, m["vertices"], m["faces"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"], w["two_sided"])
        want = dict(rows=one["rows"].astype(np.uint32), totals=one["totals"])
        _assert_state(baker, want, "the 65535th view", resolved=False)
        for _ in range(2):
            with pytest.raises(_lib.StateError):
                up.accumulate(baker, 0)
        _assert_state(baker, want, "after the refused views", resolved=False)
        baker.reset(up.F, m["cell"])   # a reset starts the count again
        up.accumulate(baker, 0)
        _assert_state(baker, want, "after a reset", resolved=False)
    finally:
        baker.destroy()
        up.destroy()


# ---------------------------------------------------------------- 3. end to end: the icosphere under the zoo's cameras, the rasterizer's own depth
def test_the_icosphere_under_rolled_steep_and_close_cameras(hip_device):
    dev = hip_device
    spheres = [T.sphere(name) for name in T.SPHERE_CAMERAS]
    s0 = spheres[0]
    F, V, w, h = s0["faces"].shape[0], s0["vertices"].shape[0], s0["width"], s0["height"]
    assert all(s["width"] == w and s["height"] == h for s in spheres)
    mesh = dict(vertices=s0["vertices"], faces=s0["faces"], colours=s0["colours"])
    cameras, images = [s["camera"] for s in spheres], [s["image"] for s in spheres]
    tolerance, min_cos, C = 0.0625, 0.1, 8
    results = {}
    for occlusion in (True, False):
        ref = T.new_state(F, C)
        for s in spheres:   # (the roll37 and below spheres are one mesh; the close camera looks at it from further off than at its own)
            depth = R.rasterize(s0["vertices"], s0["faces"], None, s["camera"], w, h, s["near"])["depth"] if occlusion else None
            T.accumulate(ref, s0["vertices"], s0["faces"], s["camera"], s["image"], depth, w, h, s["near"], tolerance, min_cos)
        texture, state = T.resolve(ref, s0["faces"], s0["colours"], V)
        got = ops.bakeTexture(dev, mesh, cameras, images, w, h, cell=C, depthTolerance=tolerance, minCos=min_cos, near=s0["near"], occlusion=occlusion)
        assert_bits_equal(got["texture"], texture, f"occlusion={occlusion}: texture")
        assert_bits_equal(got["texelState"], state, f"occlusion={occlusion}: texel states")
        assert got["textureStats"] == ref["totals"], got["textureStats"]
        L = T.layout(F, C)
        assert got["texture"].shape == (L["height"], L["width"], 4) and got["uv"].tobytes() == L["uv"].tobytes() and got["textureCell"] == C
        assert got["textureStats"]["facingAwayFaces"] > 0 and got["textureStats"]["accumulated"] > 0
        results[occlusion] = got
    with_, without = results[True]["texelState"] == 1, results[False]["texelState"] == 1
    assert np.all(without[with_]) and 0 < with_.sum() < without.sum(), "occlusion takes the silhouettes' texels out"
    # a constant photograph gives exactly that colour wherever a texel is baked or filled
    flat = [np.broadcast_to(np.array([9, 200, 31, 0], np.uint8), (h, w, 4)).copy() for _ in spheres]
    got = ops.bakeTexture(dev, dict(vertices=s0["vertices"], faces=s0["faces"]), cameras, flat, w, h, depthTolerance=tolerance, near=s0["near"])
    seen = got["texelState"] > 0
    assert seen.any() and np.all(got["texture"][seen] == np.array([9, 200, 31, 255], np.uint8))
    with pytest.raises(ValueError):
        ops.bakeTexture(dev, mesh, cameras, images[:2], w, h)
    # on the device, left there
    src = dict(vertices=dev.bufferFrom(s0["vertices"]), faces=dev.bufferFrom(s0["faces"]), colours=dev.bufferFrom(s0["colours"]), numVertices=V, numFaces=F)
    out = {}
    try:
        out = ops.bakeTexture(dev, src, [dev.bufferFrom(c) for c in cameras], [dev.bufferFrom(i) for i in images], w, h, cell=C, depthTolerance=tolerance, minCos=min_cos,
                              near=s0["near"], asBuffers=True)
        n = out["textureWidth"] * out["textureHeight"]
        assert_bits_equal(out["texture"].read(np.uint8, count=4 * n).reshape(results[True]["texture"].shape), results[True]["texture"], "asBuffers: texture")
        assert_bits_equal(out["texelState"].read(np.uint8, count=n).reshape(results[True]["texelState"].shape), results[True]["texelState"], "asBuffers: texel states")
    finally:
        ops.destroyBuffers({k: v for k, v in out.items() if isinstance(v, ops.HipBuffer) and k in ("texture", "texelState")})
        ops.destroyBuffers({k: v for k, v in src.items() if isinstance(v, ops.HipBuffer)})


# ---------------------------------------------------------------- 4. the analytic check: not through the restatement
@pytest.mark.parametrize("C", T.CELLS)
def test_the_ramp_is_reproduced_within_two_levels(hip_device, C):
    """The bound is derived in tests/test_meshtexture_reference.py: 2/512 + 0.5 + 0.5 + 0.5 < 2 levels."""
    scene = T.analytic_scene(C)
    m = scene["case"]
    w = m["views"][0]
    got = ops.bakeTexture(hip_device, dict(vertices=m["vertices"], faces=m["faces"]), [w["camera"]], [w["image"]], w["width"], w["height"], cell=C, minCos=w["min_cos"],
                          near=w["near"], occlusion=False)   # (with the occlusion test the texels on the quad's own silhouette drop out: at C = 4 all of them)
    errors, n = T.analytic_errors(scene, got["texture"], got["texelState"])
    assert n == 2 * (C - 2) * (C - 1) // 2, "every interior texel of both faces is baked"
    print(f"C = {C}: {n} interior texels, at most {errors.max():.4f} levels off the ramp")
    assert errors.max() <= 2.0, f"C = {C}: {errors.max()} levels off the ramp"


# ---------------------------------------------------------------- 5. the Trainer surface
def test_trainer_bakes_a_texture_and_extract_mesh_takes_the_option(hip_device, tmp_path):
    dev = hip_device
    cfg = harness.small_config("c2", num_points=5000, width=160, height=128, sh_deg=1, s0=0.02)
    g, sh, cameras, imgs = _views(dev, cfg, 4)
    t = _trainer(dev, cfg, g, sh, cameras, imgs, densify=False)
    lo, hi, voxel = (-2.01, -1.52, 2.03), (2.0, 1.5, 9.0), 0.11
    vol = ops.TSDFVolume.fromBounds(dev, lo, hi, voxel)
    keys = ("vertices", "faces", "colours", "keys")
    try:
        for _ in range(4):
            t.step()
        t.drain()
        t.fuseDepth(vol)
        parent = ops.weldTriangles(vol.extractTriangles(1.0))   # what extractMesh returned before it took the option
        raw = t.extractMesh(lo, hi, voxel)
        assert set(raw) == set(keys)
        for what, mesh in (("without the option", raw), ("texture=None spelled out", t.extractMesh(lo, hi, voxel, texture=None))):
            for k in keys:
                assert_bits_equal(mesh[k], parent[k], f"extractMesh {what}: {k}")
        F = raw["faces"].shape[0]
        # bakeMeshTexture = ops.bakeTexture over the trainer's own cameras and photographs
        baked = t.bakeMeshTexture(raw, depthTolerance=voxel, cell=4)
        photographs = [im["texture"].read(np.uint8).reshape(cfg.height, cfg.width, 4) for im in imgs]
        want = ops.bakeTexture(dev, raw, [c["camera"] for c in cameras], photographs, cfg.width, cfg.height, depthTolerance=voxel, cell=4)
        L = ops.textureLayout(F, 4)
        assert baked["views"] == [0, 1, 2, 3] and baked["textureStats"] == want["textureStats"] and 0 < baked["textureStats"]["bakedTexels"]
        assert_bits_equal(baked["texture"], want["texture"], "bakeMeshTexture: texture")
        assert_bits_equal(baked["texelState"], want["texelState"], "bakeMeshTexture: texel states")
        assert baked["texture"].shape == (L["height"], L["width"], 4) and baked["texelState"].shape == (L["height"], L["width"])
        assert baked["uv"].shape == (F, 3, 2) and baked["uv"].tobytes() == L["uv"].tobytes()
        for k in keys:
            assert_bits_equal(baked[k], raw[k], f"bakeMeshTexture leaves {k}")
        with pytest.raises(TypeError):
            t.bakeMeshTexture(raw, depthTolerence=voxel)
        # extractMesh(texture=...) textures last, on the final mesh, after bake
        base = t.extractMesh(lo, hi, voxel, minTriangles=20, simplify=2 * voxel, normals=True, bake=True)
        got = t.extractMesh(lo, hi, voxel, minTriangles=20, simplify=2 * voxel, normals=True, bake=True, texture=dict(depthTolerance=voxel))
        for k in ("vertices", "faces", "normals", "colours"):
            assert_bits_equal(got[k], base[k], f"extractMesh(texture): {k}")
        again = t.bakeMeshTexture(base, depthTolerance=voxel)
        assert_bits_equal(got["texture"], again["texture"], "extractMesh(texture): texture")
        assert got["textureStats"] == again["textureStats"] and got["bakeStats"] == base["bakeStats"] and got["textureCell"] == 8
        F2 = got["faces"].shape[0]
        assert got["uv"].shape == (F2, 3, 2) and got["texture"].shape[:2] == (got["textureHeight"], got["textureWidth"]) and F2 < F
        # the OBJ a viewer opens loads back exactly
        path = str(tmp_path / "scene.obj")
        loaders.saveMeshOBJ(path, got)
        back = loaders.loadMeshOBJ(path)
        for k in ("vertices", "faces", "uv", "texture", "normals"):
            assert back[k].dtype == got[k].dtype and back[k].tobytes() == np.ascontiguousarray(got[k]).tobytes(), f"OBJ round trip: {k}"
    finally:
        vol.destroy()
        t.destroy()
