"""Vertex colours baked from photographs, restated: ``meshraster_ref.project`` and numpy float32 scalars -- one operation per rounding
of include/webdgs.h's definition, in its order -- for the position and the weight, Python integers for everything else, and a loop over the vertices.
``accumulate`` adds one view to a state, ``resolve`` turns a state into colours; ``CASES`` are the crafted meshes and views the CPU and the GPU tests share."""
import functools
import hashlib

import numpy as np

import camzoo
import meshraster_ref as mr
from meshraster_ref import at, crafted_camera

F32 = np.float32
STATS = ("usable", "inImage", "visible", "accumulated", "viewportMismatch", "bakedVertices")
NEAR = 0.01


# ---------------------------------------------------------------- the definition
def new_state(V):
    """The state after ``reset(V)``: ``sums`` and ``views`` as lists of Python integers, the totals as a dict."""
    return dict(V=int(V), sums=[[0, 0, 0, 0] for _ in range(V)], views=[0] * V, totals=dict.fromkeys(STATS, 0))


def cosine(camera, v, n):
    """Step 4's ``c`` for a view-space position ``v`` and a world-space normal ``n`` (float32 arrays of 3): a numpy float32 scalar."""
    c = np.ascontiguousarray(camera, F32).reshape(-1)
    v, n = np.ascontiguousarray(v, F32), np.ascontiguousarray(n, F32)
    with np.errstate(all="ignore"):
        nv = [(c[i] * n[0] + c[4 + i] * n[1]) + c[8 + i] * n[2] for i in range(3)]
        dot = (nv[0] * v[0] + nv[1] * v[1]) + nv[2] * v[2]
        nn = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]
        vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        out = (-dot) / np.sqrt(nn * vv)
    assert isinstance(out, np.float32)
    return out


def weight(camera, v, n, min_cos):
    """Step 4's ``Q`` (0: the vertex is skipped)."""
    c = cosine(camera, v, n)
    if not np.isfinite(c) or c < F32(min_cos):
        return 0
    q = np.rint((F32(1) if c > F32(1) else c) * F32(256))
    assert isinstance(q, np.float32)
    return int(q)


def footprint(xs, ys, W, H):
    """Step 2: ``None`` outside the image, else ``(texels, weights)`` -- the four ``(i, j)`` in the order (i0, j0), (i1, j0), (i0, j1), (i1, j1) and their
    integer weights, which sum to 65536."""
    if not (0 <= xs <= 256 * (W - 1) and 0 <= ys <= 256 * (H - 1)):
        return None
    i0, a, j0, b = xs >> 8, xs & 255, ys >> 8, ys & 255
    i1, j1 = min(i0 + 1, W - 1), min(j0 + 1, H - 1)
    return [(i0, j0), (i1, j0), (i0, j1), (i1, j1)], [(256 - a) * (256 - b), a * (256 - b), (256 - a) * b, a * b]


def sample(image, texels, weights):
    """Step 5: ``(S, s)`` per colour channel, lists of three Python integers."""
    S = [sum(w * int(image[j, i, ch]) for (i, j), w in zip(texels, weights)) for ch in range(3)]
    return S, [(x + 128) >> 8 for x in S]


def accumulate(state, vertices, normals, camera, image, depth, width, height, near=NEAR, depth_tolerance=0.0625, min_cos=0.0):
    """One view added to ``state``, in place."""
    W, H = int(width), int(height)
    cam = np.ascontiguousarray(camera, F32).reshape(-1)
    t = state["totals"]
    if not (cam[64] == F32(W) and cam[65] == F32(H)):
        t["viewportMismatch"] += 1
        return state
    p = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    assert p.shape[0] == state["V"]
    n = None if normals is None else np.ascontiguousarray(normals, F32).reshape(-1, 3)
    img = np.ascontiguousarray(image, np.uint8).reshape(H, W, 4)
    dep = None if depth is None else np.ascontiguousarray(depth, F32).reshape(H, W)
    X, Y, view, usable = mr.project(p, cam, W, H, near)
    for k in range(p.shape[0]):
        if not usable[k]:
            continue
        t["usable"] += 1
        fp = footprint(X[k] - 128, Y[k] - 128, W, H)
        if fp is None:
            continue
        t["inImage"] += 1
        texels, weights = fp
        if dep is not None:
            z = view[k, 2]
            with np.errstate(all="ignore"):
                d = [dep[j, i] for i, j in texels]
                if not all(bool(np.isfinite(x) and x > 0 and np.abs(z - x) <= F32(depth_tolerance)) for x in d):
                    continue
        t["visible"] += 1
        Q = 256 if n is None else weight(cam, view[k], n[k], min_cos)
        if Q == 0:
            continue
        t["accumulated"] += 1
        _, s = sample(img, texels, weights)
        assert all(x <= 65280 for x in s)
        row = state["sums"][k]
        for ch in range(3):
            row[ch] += Q * s[ch]
        row[3] += Q
        state["views"][k] = min(state["views"][k] + 1, 2 ** 32 - 1)
    return state


def resolve(state, fallback=None, min_views=1, min_weight=1):
    """``(colours u8[V,4], baked bool[V])``, and ``bakedVertices`` of the state's totals set."""
    V = state["V"]
    colours = np.zeros((V, 4), np.uint8) if fallback is None else np.array(fallback, np.uint8).reshape(V, 4)
    baked = np.zeros(V, bool)
    for k in range(V):
        R, G, B, Wt = state["sums"][k]
        if state["views"][k] >= max(int(min_views), 1) and Wt >= max(int(min_weight), 1):
            baked[k] = True
            colours[k] = [min(255, (x + 128 * Wt) // (256 * Wt)) for x in (R, G, B)] + [255]
    state["totals"]["bakedVertices"] = int(baked.sum())
    return colours, baked


def arrays(state):
    """``(sums u64[V,4], views u32[V])`` of a state, as ``MeshColourBaker.read`` hands them out."""
    return np.array(state["sums"], np.uint64).reshape(state["V"], 4), np.array(state["views"], np.uint32)


# ---------------------------------------------------------------- the crafted cases
# A case: dict(vertices f32[V,3], normals f32[V,3] | None, views: [dict(camera, image u8[H,W,4], depth f32[H,W] | None, width, height, near, depth_tolerance,
# min_cos)], fallback u8[V,4] | None, min_views, min_weight).  The normals are used by every view of the case or by none.
def _view(image, depth=None, camera=None, near=NEAR, depth_tolerance=0.0625, min_cos=0.0):
    image = np.ascontiguousarray(image, np.uint8)
    H, W = image.shape[:2]
    return dict(camera=crafted_camera(W, H) if camera is None else np.ascontiguousarray(camera, F32), image=image,
                depth=None if depth is None else np.ascontiguousarray(depth, F32).reshape(H, W), width=W, height=H, near=near, depth_tolerance=depth_tolerance,
                min_cos=min_cos)


def _case(vertices, views, normals=None, fallback=None, min_views=1, min_weight=1):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    return dict(vertices=v, normals=None if normals is None else np.ascontiguousarray(normals, F32).reshape(v.shape[0], 3), views=views,
                fallback=None if fallback is None else np.ascontiguousarray(fallback, np.uint8).reshape(v.shape[0], 4), min_views=min_views, min_weight=min_weight)


def noise_image(W, H, seed):
    return np.random.default_rng(8000 + seed).integers(0, 256, (H, W, 4)).astype(np.uint8)


def ramp_image(W, H):
    """T(i, j) = 3 i + 2 j in red, 255 - that in green, j in blue: bilinear interpolation of it is exact."""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = 3 * i + 2 * j
    assert t.max() <= 255
    return np.stack([t, 255 - t, j, np.full_like(t, 77)], axis=2).astype(np.uint8)


def pixel(xs, ys, z, W, H):
    """The world position the crafted camera puts at X' = xs, Y' = ys (1/256 texel units from the centre of texel (0, 0)) and depth z."""
    return at((xs + 128) / 256.0, (ys + 128) / 256.0, z, W, H)


def _borders(W, H):
    """The edges of step 2 in x and in y, and of step 1: the guard band, the near plane, a NaN.  EXPECT holds the totals."""
    def make():
        xm, ym = 256 * (W - 1), 256 * (H - 1)
        cx, cy = xm // 2 + 3, ym // 2 + 5
        v = [pixel(0, cy, 1.0, W, H), pixel(xm, cy, 1.0, W, H), pixel(-1, cy, 1.0, W, H), pixel(xm + 1, cy, 1.0, W, H),
             pixel(cx, 0, 2.0, W, H), pixel(cx, ym, 2.0, W, H), pixel(cx, -1, 2.0, W, H), pixel(cx, ym + 1, 2.0, W, H),
             pixel(0, 0, 1.5, W, H), pixel(xm, ym, 1.5, W, H),
             [(16384.0 - W / 2) * 2 / W, 0.0, 1.0], [(16384.0 + 2.0 ** -9 - W / 2) * 2 / W, 0.0, 1.0], [-(16384.0 + W / 2) * 2 / W, 0.0, 1.0],
             [-(16384.0 + 2.0 ** -9 + W / 2) * 2 / W, 0.0, 1.0], [0.0, (16384.0 + 2.0 ** -9 + H / 2) * 2 / H, 1.0],
             [0.0, 0.0, F32(NEAR)], [0.0, 0.0, np.nextafter(F32(NEAR), F32(0))], [float("nan"), 0.0, 1.0], [0.0, 0.0, float("inf")]]
        return _case(v, [_view(noise_image(W, H, W + H))], fallback=mr._rainbow(len(v), 11))
    return make


def _depth_rule():
    """One vertex between the four texels of a 2 x 2 image, at depths round a depth image of 2 + 2^-4 under the tolerance 2^-4 (every difference is exact),
    then under the tolerance 0, then with one texel absent, NaN, infinite or negative."""
    W = H = 2
    d, tol = F32(2.0625), 0.0625
    zs = [F32(2.0), np.nextafter(F32(2.0), F32(0)), F32(2.125), np.nextafter(F32(2.125), F32(3)), d, np.nextafter(d, F32(0)), np.nextafter(d, F32(3))]
    v = [pixel(100, 60, float(z), W, H) for z in zs]
    views = [_view(noise_image(W, H, 1), np.full((H, W), d), depth_tolerance=tol), _view(noise_image(W, H, 2), np.full((H, W), d), depth_tolerance=0.0)]
    for k, bad in enumerate((0.0, float("nan"), float("inf"), -2.0625)):
        for where in ((k % 2, k // 2), ((k + 1) % 2, 1 - k // 2)):
            image = np.full((H, W), d)
            image[where[1], where[0]] = bad
            views.append(_view(noise_image(W, H, 3 + k), image, depth_tolerance=tol))
    return _case(v, views)


def _find_cosine_above_one():
    """A depth z and a normal scale for which c = z s / sqrt((s s)(z z)) rounds above 1."""
    cam = crafted_camera(2, 2)
    rng = np.random.default_rng(5)
    for _ in range(10000):
        z, s = F32(rng.uniform(1.0, 3.0)), F32(rng.uniform(0.5, 2.0))
        if cosine(cam, [0, 0, z], [0, 0, -s]) > F32(1):
            return float(z), float(s)
    raise AssertionError("no cosine above 1 found")


def _weight_rule():
    """One 2 x 2 view per threshold over vertices with crafted normals: a cosine equal to min_cos and one ulp below it, a cosine above 1 by rounding, a
    back-facing, a zero and a NaN normal, and Q rounding to 0."""
    W = H = 2
    cam = crafted_camera(W, H)
    z1, s1 = _find_cosine_above_one()
    v = [pixel(100, 60, 2.0, W, H), [0.0, 0.0, z1], pixel(30, 200, 1.5, W, H), pixel(30, 200, 1.5, W, H), pixel(30, 200, 1.5, W, H), [0.0, 0.0, 1.0], [0.0, 0.0, 1.0],
         [0.0, 0.0, 1.0]]
    nan = float("nan")
    n = [[0.3, -0.2, -0.8], [0.0, 0.0, -s1], [0.1, 0.1, 1.0], [0.0, 0.0, 0.0], [nan, 0.0, -1.0], [1.0, 0.0, -0.001], [1.0, 0.0, -0.001953125], [0.0, 1.0, -0.0059]]
    c = cosine(cam, np.asarray(v[0], F32), np.asarray(n[0], F32))   # (the crafted view is the identity: view space is world space)
    assert 0 < c < 1
    image = noise_image(W, H, 9)
    views = [_view(image, min_cos=float(c)), _view(image, min_cos=float(np.nextafter(c, F32(2)))), _view(image, min_cos=0.0), _view(image, min_cos=1.0)]
    return _case(v, views, normals=n)


def _random(V, W, H, depth, normals, seed, views=2):
    """V vertices scattered over and a little round a W x H image at depths round 2, views with noise photographs and noisy depth images."""
    def make():
        rng = np.random.default_rng(100 + seed)
        sx, sy, z = rng.uniform(-0.5, W + 0.5, V), rng.uniform(-0.5, H + 0.5, V), 2.0 + rng.uniform(-0.05, 0.05, V)
        v = np.array([at(a, b, c, W, H) for a, b, c in zip(sx, sy, z)], F32).reshape(V, 3)
        n = None
        if normals:
            n = rng.normal(0.0, 1.0, (V, 3))
            n[:, 2] -= 1.0   # (more of them face the camera)
        vs = [_view(noise_image(W, H, seed + 10 * k), (2.0 + rng.uniform(-0.04, 0.04, (H, W))) if depth else None, depth_tolerance=0.0625, min_cos=0.1 * k)
              for k in range(views)]
        return _case(v, vs, normals=n, fallback=mr._rainbow(V, 12 + seed), min_views=1 + seed % 2)
    return make


def _mismatch():
    W = H = 4
    v = [pixel(300, 300, 1.0, W, H), pixel(100, 500, 1.0, W, H)]
    return _case(v, [_view(noise_image(W, H, 4), camera=crafted_camera(W, H, block_size=(8, 8))), _view(noise_image(W, H, 5))], fallback=mr._rainbow(2, 13))


SIZES = ((1, 1), (2, 2), (5, 3), (67, 45))
COUNTS = (0, 1, 255, 256, 257, 1000)
FORMS = ((False, False), (False, True), (True, False), (True, True))   # (depth, normals): the kernel's four forms


def _random_cases():
    """Every vertex count in every form; the image sizes go round, so that each count meets each size but one."""
    out = {}
    for a, V in enumerate(COUNTS):
        for b, (depth, normals) in enumerate(FORMS):
            W, H = SIZES[(a + b) % 4]
            out[f"random-{V}-{W}x{H}{'-depth' if depth else ''}{'-normals' if normals else ''}"] = _random(V, W, H, depth, normals, 4 * a + b, views=3 if V == 257 else 2)
    return out


CASES = dict({"borders-1x1": _borders(1, 1), "borders-2x2": _borders(2, 2), "borders-5x3": _borders(5, 3), "borders-67x45": _borders(67, 45),
              "depth-rule": _depth_rule, "weight-rule": _weight_rule, "viewport-mismatch": _mismatch}, **_random_cases())
THREE_VIEWS = "random-257-67x45-depth-normals"   # the case whose views are permuted
# what the definition gives, where the case is about it: the totals before the resolve
EXPECT = {
    # usable: the ten placed by `pixel`, the two on the guard band's edge and the one on the near plane; in the image: six of the ten -- those at -1 and one
    # past the far edge are outside -- and the one on the near plane, which sits in the middle
    "borders-2x2": dict(usable=13, inImage=7, visible=7, accumulated=7, viewportMismatch=0),
    # tolerance 2^-4: z = 2 and 2.125 and the three round d pass; tolerance 0: z = d alone; a bad texel: nothing
    "depth-rule": dict(usable=7 * 10, inImage=7 * 10, visible=5 + 1, accumulated=5 + 1),
    "viewport-mismatch": dict(usable=2, inImage=2, visible=2, accumulated=2, viewportMismatch=1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name; computed once and shared: callers leave it unchanged."""
    m = CASES[name]()
    for a in [m["vertices"], m["normals"], m["fallback"]] + [x for v in m["views"] for x in v.values()]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def run(m, order=None):
    """``dict(sums, views, totals, colours, baked)``: the views of case ``m`` accumulated in ``order`` (default: as listed) and resolved."""
    V = m["vertices"].shape[0]
    state = new_state(V)
    for k in (range(len(m["views"])) if order is None else order):
        w = m["views"][k]
        accumulate(state, m["vertices"], m["normals"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"])
    before = dict(state["totals"])
    colours, baked = resolve(state, m["fallback"], m["min_views"], m["min_weight"])
    sums, views = arrays(state)
    return dict(sums=sums, views=views, totals=state["totals"], totalsBeforeResolve=before, colours=colours, baked=baked)


@functools.lru_cache(maxsize=None)
def expected(name):
    """``run`` of that case; computed once and shared: callers leave it unchanged."""
    out = run(case(name))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def digest(result):
    """sha256 over sums, views, colours, the mask as bytes and the totals (what a host's run script prints)."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(result["sums"], np.uint64).tobytes())
    h.update(np.ascontiguousarray(result["views"], np.uint32).tobytes())
    h.update(np.ascontiguousarray(result["colours"], np.uint8).tobytes())
    h.update(np.ascontiguousarray(result["baked"]).astype(np.uint8).tobytes())
    h.update(np.array([result["totals"][k] for k in STATS], np.uint64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- the icosphere under the zoo's cameras
SPHERE_CAMERAS = ("roll37", "below", "close")


@functools.lru_cache(maxsize=None)
def sphere(camera_name):
    """``meshraster_ref``'s 162-vertex icosphere case under that camera, with its outward normals and a noise photograph."""
    m = mr.case(f"sphere-{camera_name}")
    v = np.asarray(m["vertices"], np.float64)
    centre = (v.max(axis=0) + v.min(axis=0)) / 2
    n = v - centre
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    image = noise_image(m["width"], m["height"], 40 + SPHERE_CAMERAS.index(camera_name))
    for a in (n, image):
        a.setflags(write=False)
    return dict(m, normals=n, image=image)
