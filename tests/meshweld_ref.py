"""Welding a triangle soup, restated without numpy's unique: Python's stable ``sorted`` on (key, slot), then one loop for the heads and
the ranks.  ``weld`` takes and returns what ``ops.weldTriangles`` does; ``CASES`` are the crafted soups the CPU and the GPU tests share."""
import functools

import numpy as np

U64_MAX = 2 ** 64 - 1


def weld(tri):
    """``dict(vertices f32[V,3], faces u32[F,3], colours u8[V,3] | None, keys u64[V])``: the distinct keys ascending, every slot's rank, and for every
    distinct key the position and colour of the LOWEST slot that carries it."""
    keys = [int(k) for k in np.asarray(tri["keys"], np.uint64).reshape(-1)]
    S = len(keys)
    positions = np.ascontiguousarray(tri["positions"], np.float32).reshape(-1, 3)
    colours = None if tri.get("colours") is None else np.asarray(tri["colours"], np.uint8).reshape(-1, 4)
    order = sorted(range(S), key=lambda s: (keys[s], s))
    faces = np.zeros(S, np.uint32)
    heads, uniq = [], []
    for i, s in enumerate(order):
        if i == 0 or keys[s] != keys[order[i - 1]]:
            heads.append(s)
            uniq.append(keys[s])
        faces[s] = len(heads) - 1
    heads = np.asarray(heads, np.int64)
    return dict(vertices=np.ascontiguousarray(positions[heads]), faces=faces.reshape(-1, 3),
                colours=None if colours is None else np.ascontiguousarray(colours[heads, :3]), keys=np.asarray(uniq, np.uint64))


def soup(keys, seed=0, positions=None, colours=None):
    """A soup around ``keys`` (S of them, S a multiple of 3): every slot gets position and colour bits of its own unless they are given, so that equal keys
    carry DIFFERENT payloads and only the lowest-slot rule decides which one a vertex shows."""
    k = np.ascontiguousarray(keys, np.uint64).reshape(-1, 3)
    F = k.shape[0]
    rng = np.random.default_rng(1000 + seed)
    if positions is None:
        positions = rng.integers(0, 2 ** 32, (F, 3, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)   # any bit pattern, NaNs included
    if colours is None:
        colours = rng.integers(0, 256, (F, 3, 4), dtype=np.uint64).astype(np.uint8)
    return dict(keys=k, positions=np.ascontiguousarray(positions, np.float32).reshape(F, 3, 3), colours=np.ascontiguousarray(colours, np.uint8).reshape(F, 3, 4))


def _random_u64(rng, n):
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64)


def _empty():
    return soup(np.zeros(0, np.uint64))


def _one_distinct():
    return soup(np.array([5, 3, 9], np.uint64))


def _one_equal():
    return soup(np.array([7, 7, 7], np.uint64))


def _extremes():
    return soup(np.array([0, U64_MAX, 5, U64_MAX, 0, 2 ** 63, 5, 0, U64_MAX, 2 ** 63 - 1, 1, U64_MAX - 1], np.uint64), 1)


def _all_equal():
    return soup(np.full(30000, 0x0123456789ABCDEF, np.uint64), 2)


def _top_byte():
    rng = np.random.default_rng(3)
    return soup(np.uint64(0x00C0FFEE12345678) | (rng.integers(0, 256, 6000, dtype=np.uint64) << np.uint64(56)), 3)


def _low_byte():
    rng = np.random.default_rng(4)
    return soup(np.uint64(0xFEDCBA9876543200) | rng.integers(0, 256, 6000, dtype=np.uint64), 4)


def _random_u64_case():
    # S = 20 481: one past a multiple of 4 096; each key about six times, the slots shuffled
    rng = np.random.default_rng(5)
    S = 3 * 6827
    values = _random_u64(rng, S // 6)
    for byte in range(8):
        assert np.unique((values >> np.uint64(8 * byte)) & np.uint64(255)).size > 1
    return soup(rng.permutation(values[np.arange(S) % values.size]), 5)


def _heavy_bin():
    # in the first pass one digit bin holds every key but one; the other bytes vary
    rng = np.random.default_rng(6)
    keys = (_random_u64(rng, 9000) & ~np.uint64(255)) | np.uint64(0x11)
    keys[4321] = (keys[4321] & ~np.uint64(255)) | np.uint64(0x12)
    return soup(keys, 6)


def _lowest_slot():
    # four distinct keys over 30 000 slots; positions[s] = (s, s, s) and colours[s] spell s as well
    rng = np.random.default_rng(7)
    S = 30000
    keys = np.array([2 ** 40 + 3, 17, 2 ** 63 + 1, 17 + 2 ** 20], np.uint64)[rng.integers(0, 4, S)]
    s = np.arange(S)
    colours = np.stack([s & 255, (s >> 8) & 255, (s * 7) & 255, (s * 13) & 255], axis=1)
    return soup(keys, 7, positions=np.repeat(s.astype(np.float32), 3), colours=colours)


def _scan_blocks():
    # F = 100 000 with random 20-bit keys: 74 workgroups of 4 096 pairs, a digit table of 18 944 words, five blocks of the scan
    rng = np.random.default_rng(8)
    return soup(rng.integers(0, 2 ** 20, 300000, dtype=np.uint64), 8)


CASES = {"empty": _empty, "one-distinct": _one_distinct, "one-equal": _one_equal, "extremes": _extremes, "all-equal": _all_equal, "top-byte": _top_byte,
         "low-byte": _low_byte, "random-u64": _random_u64_case, "heavy-bin": _heavy_bin, "lowest-slot": _lowest_slot, "scan-blocks": _scan_blocks}
# the radix passes (of eight) whose digit differs somewhere, where the case is about them
PASSES_RUN = {"empty": 0, "one-equal": 0, "all-equal": 0, "top-byte": 1, "low-byte": 1, "random-u64": 8, "heavy-bin": 8, "scan-blocks": 3}


@functools.lru_cache(maxsize=None)
def case(name):
    """The soup of that name; computed once and shared: callers leave it unchanged."""
    tri = CASES[name]()
    for a in tri.values():
        a.setflags(write=False)
    return tri


def digest(mesh):
    """sha256 over the mesh's arrays in a fixed order (what bindings/napi/meshweld_run.js prints)."""
    import hashlib
    h = hashlib.sha256()
    for k in ("vertices", "faces", "colours", "keys"):
        if mesh[k] is not None:
            h.update(np.ascontiguousarray(mesh[k]).tobytes())
    return h.hexdigest()
