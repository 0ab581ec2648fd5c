"""Per-face visibility over views, the rule on its counters and the face filter restated in plain numpy (include/webdgs.h):
``np.bincount`` over the counted pixels, boolean masks for the rule, a cumulative sum for the compaction.  Every output is an integer array (or a gather
of the input's floats); the GPU tests compare bytes.  Also the crafted face images the CPU and the GPU tests share."""
import numpy as np

EMPTY = 0xFFFFFFFF
MAX_SIZE = 8192   # WDGS_MESH_RASTER_MAX_SIZE


def agrees(mesh_depth, model_depth, weight_sum, min_weight_sum, threshold):
    """bool per pixel: both depths present by ``wdgs_depth_agreement``'s rule and ``|a - b| <= threshold``, every operation in float32."""
    a, b = np.asarray(mesh_depth, np.float32).reshape(-1), np.asarray(model_depth, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        has_a = (a > 0) & (a < np.float32(np.inf))
        has_b = (b > 0) & (b < np.float32(np.inf))
        if weight_sum is not None:
            has_b &= np.asarray(weight_sum, np.float32).reshape(-1) >= np.float32(min_weight_sum)
        d = np.abs((a - b).astype(np.float32))
        return has_a & has_b & (d <= np.float32(threshold))


class Accumulator:
    """``wdgs_face_visibility`` for F faces: ``counters`` u32[F,3] = {pixels, agreeing, views}, ``views``, ``foreign``, ``counted``, ``agreeing``."""

    def __init__(self, num_faces):
        self.reset(num_faces)

    def reset(self, num_faces):
        self.F = int(num_faces)
        assert 0 <= self.F < 2 ** 31
        self.counters = np.zeros((self.F, 3), np.uint32)
        self.views = self.foreign = self.counted = self.agreeing = 0

    def would_overflow(self, width, height):
        return (self.views + 1) * int(width) * int(height) >= 2 ** 32

    def accumulate(self, face_image, mesh_depth=None, model_depth=None, weight_sum=None, min_weight_sum=0.0, threshold=0.05):
        """One view; the image in any shape (only counts matter).  Returns ``(counted, agreeing, foreign)`` of the view."""
        f = np.ascontiguousarray(face_image, np.uint32).reshape(-1)
        assert (mesh_depth is None) == (model_depth is None)
        assert not self.would_overflow(f.size, 1)
        counted = f.astype(np.int64) < self.F
        foreign = ~counted & (f != np.uint32(EMPTY))
        agree = counted.copy() if mesh_depth is None else counted & agrees(mesh_depth, model_depth, weight_sum, min_weight_sum, threshold)
        pixels = np.bincount(f[counted].astype(np.int64), minlength=self.F)
        agreeing = np.bincount(f[agree].astype(np.int64), minlength=self.F)
        total = self.counters.astype(np.int64)
        total[:, 0] += pixels
        total[:, 1] += agreeing
        total[:, 2] += pixels > 0
        assert total.max(initial=0) < 2 ** 32
        self.counters = total.astype(np.uint32)
        self.views += 1
        self.foreign += int(foreign.sum())
        self.counted += int(counted.sum())
        self.agreeing += int(agree.sum())
        return int(counted.sum()), int(agree.sum()), int(foreign.sum())

    def stats(self):
        return dict(views=self.views, foreignPixels=self.foreign, countedPixels=self.counted, agreeingPixels=self.agreeing)


def fraction_q16(fraction):
    assert 0.0 <= float(fraction) <= 1.0
    return int(np.rint(np.float64(fraction) * 65536.0))


def flags(counters, min_pixels=1, min_views=1, min_agreeing=0, min_agreeing_q16=0):
    """u8[F]: the rule, written face by face in Python integers (unlike the product's)."""
    c = np.asarray(counters, np.uint32).reshape(-1, 3)
    out = np.zeros(c.shape[0], np.uint8)
    for i, (pixels, agreeing, views) in enumerate(c.tolist()):
        out[i] = 1 if (pixels >= min_pixels and views >= min_views and agreeing >= min_agreeing and agreeing * 65536 >= min_agreeing_q16 * pixels) else 0
    return out


def filter_faces(mesh, keep):
    """``dict(vertices, faces, vertexMap, faceMap, invalidFaces)`` and ``colours`` / ``keys`` where ``mesh`` has them: a face is kept when its flag is
    non-zero and its indices are vertices, a vertex exactly when a kept face names it; kept faces in their order, kept vertices in ascending original
    index, faces rewritten."""
    faces = np.ascontiguousarray(mesh["faces"], np.uint32).reshape(-1, 3)
    vertices = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1, 3)
    V = vertices.shape[0]
    valid = np.all(faces.astype(np.int64) < V, axis=1) if faces.size else np.zeros(0, bool)
    fkeep = valid & (np.asarray(keep).reshape(-1) != 0)
    vkeep = np.zeros(V, bool)
    vkeep[faces[fkeep].astype(np.int64).reshape(-1)] = True
    vmap, fmap = np.flatnonzero(vkeep).astype(np.uint32), np.flatnonzero(fkeep).astype(np.uint32)
    new_index = np.cumsum(vkeep) - vkeep
    out = dict(vertices=vertices[vmap], faces=new_index[faces[fmap].astype(np.int64)].astype(np.uint32).reshape(-1, 3), vertexMap=vmap, faceMap=fmap,
               invalidFaces=int((~valid).sum()))
    for name in ("colours", "keys"):
        if name in mesh:
            out[name] = None if mesh[name] is None else np.ascontiguousarray(np.asarray(mesh[name])[vmap])
    return out


# ---------------------------------------------------------------- the crafted face images: name -> (F, width, height, u32[height * width])
def _one_face(w, h, F=3, f=1):
    return F, w, h, np.full(w * h, f, np.uint32)


def _alternating(w=67, h=45):
    return 2, w, h, (np.arange(w * h) % 2).astype(np.uint32)


def _run_lengths():
    """Runs of 1, 2, ..., 130 pixels, the face index stepping through 0 .. 6 with an empty run now and then: 8515 pixels as 131 x 65."""
    keys = [(n % 8) if n % 8 != 7 else EMPTY for n in range(1, 131)]
    img = np.concatenate([np.full(n, k, np.uint32) for n, k in zip(range(1, 131), keys)])
    assert img.size == 131 * 65
    return 7, 131, 65, img


def _random(F, w=128, h=96, seed=17):
    return F, w, h, np.random.default_rng(seed).integers(0, F, w * h).astype(np.uint32)


def _foreign(w=61, h=37, F=9, seed=23):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, F, w * h).astype(np.uint32)
    kind = rng.integers(0, 8, w * h)
    for k, value in ((0, F), (1, 2 ** 31), (2, 0xFFFFFFFE), (3, EMPTY)):
        img[kind == k] = value
    return F, w, h, img


IMAGES = {
    "no-faces": lambda: (0, 16, 9, np.where(np.arange(144) % 3 == 0, 5, EMPTY).astype(np.uint32)),
    "one-pixel": lambda: (4, 1, 1, np.array([2], np.uint32)),
    "all-empty": lambda: (5, 33, 7, np.full(231, EMPTY, np.uint32)),
    "one-face-67x45": lambda: _one_face(67, 45),
    "one-face-256x256": lambda: _one_face(256, 256),
    "alternating": _alternating,
    "run-lengths": _run_lengths,
    "random-5": lambda: _random(5),
    "random-100000": lambda: _random(100000),
    "foreign": _foreign,
}

_cache = {}


def image(name):
    """``(F, width, height, image)`` of a named image, computed once and shared (read-only)."""
    if name not in _cache:
        F, w, h, img = IMAGES[name]()
        img.setflags(write=False)
        _cache[name] = (F, w, h, img)
    return _cache[name]
