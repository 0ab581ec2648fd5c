"""Crafted key streams for the forward pass's tile sort (webdgs_amd/csrc/sort.hip) and their exact reference.  Plain numpy: nothing here
needs a GPU or the library.

A stream is (keys, values): key = (tile + 1) << 16 | depth16, values distinct u32 that are neither the index nor sorted.  The expected
result is the stable sort of the 32-bit keys, the expected range table a lower-bound search on the sorted keys.  There are no tolerances.

The *segment zoo* is one list of named per-tile cases, each a multiset of depth16 values in a fixed emission order, written for the
constants below (tests/test_sort_cases.py reads them out of sort.hip and fails when one of them moves: the edges must move with it).
"""
import numpy as np

# What the zoo was written for (sort.hip)
SEG_CAP = 2048           # a tile with more entries takes seg_pass_global, in trips of GLOBAL_TRIP entries
SEG_WIDE_BITS = 10       # one-pass routes: span < 2^8, < 2^9, < 2^SEG_WIDE_BITS; a wider span takes two 8-bit passes in LDS
SORT_ITEMS_MAX = 16      # keys per thread of a partition of a large sorter (a small one: SORT_ITEMS_SMALL)
SORT_ITEMS_SMALL = 4
SORT_THREADS = 256
SMALL_SORTER_MAX = 8 << 20   # capacity up to which a sorter is a small one
GLOBAL_TRIP = 1024
SCAN_ROWS_STEP = 1024    # partitions per iteration of sort_scan_rows
EMPTY = 0xFFFFFFFF

BRANCHES = ("lds-8", "lds-9", "lds-10", "lds-2x8", "global")
ONE_PASS_BITS = {"lds-8": 8, "lds-9": 9, "lds-10": SEG_WIDE_BITS}

LDS_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048)
LDS_SPANS = (0, 1, 255, 256, 511, 512, 1023, 1024, 65535)
ORDER_LENGTHS = (300, 2048)
ORDER_SPANS = (255, 511, 1023, 40000)   # one per LDS branch
GLOBAL_LENGTHS = (2049, 3071, 3072, 3073, 4096, 4097, 10_000)
GLOBAL_DISTRIBUTIONS = ("uniform", "equal", "high-byte", "low-byte", "descending")


def classify(n, span):
    """The branch of segment_sort_kernel a tile of n entries with depth span (max - min) takes."""
    if n > SEG_CAP:
        return "global"
    if span < (1 << 8):
        return "lds-8"
    if span < (1 << 9):
        return "lds-9"
    if span < (1 << SEG_WIDE_BITS):
        return "lds-10"
    return "lds-2x8"


def _bins_for(span):
    b = classify(1, span)
    return 1 << ONE_PASS_BITS.get(b, 8)


def _minimum(span, position):
    """Where [min, min + span] lies: 0 at the bottom, 1 at the top, 2 across a multiple of the bin count of the branch the span takes
    (so that a digit taken from the raw depth bits, without the subtraction of the minimum, wraps inside the segment)."""
    if position == 0 or span == 0xFFFF:
        return 0
    if position == 1:
        return 0xFFFF - span
    bins = _bins_for(span)
    k = max(1, min(37, (0xFFFF - span) // bins))   # a multiple k * bins with room for the span on both sides
    return max(0, k * bins - (span + 1) // 2)


def _lds_segments(rng):
    out = []
    for i, n in enumerate(LDS_LENGTHS):
        for j, span in enumerate(LDS_SPANS):
            if span > 0 and n < 2:
                continue
            lo = _minimum(span, (i + j) % 3)   # every span meets every position, at lengths that differ
            d = rng.integers(lo, lo + span + 1, n, dtype=np.int64)
            if span > 0:   # both extremes are always there
                a, b = rng.choice(n, 2, replace=False)
                d[a], d[b] = lo, lo + span
            out.append((f"lds n={n} span={span} min={lo:#06x}", d))
    return out


def _order_segments(rng):
    out = []
    for n in ORDER_LENGTHS:
        for span in ORDER_SPANS:
            lo = _minimum(span, 2)
            body = np.concatenate([[lo, lo + span], rng.integers(lo, lo + span + 1, n - 2, dtype=np.int64)])
            asc = np.sort(body, kind="stable")
            two = np.where(rng.random(n) < 0.5, lo, lo + span)
            two[0], two[-1] = lo + span, lo
            last = np.full(n, lo + span, np.int64)
            last[-1] = lo
            for name, d in (("ascending", asc), ("descending", asc[::-1].copy()), ("two-values", two), ("all-equal-but-last", last)):
                out.append((f"order {name} n={n} span={span} min={lo:#06x}", d))
    return out


def _global_segments(rng):
    out = []
    for i, n in enumerate(GLOBAL_LENGTHS):
        for dist in (GLOBAL_DISTRIBUTIONS[(i + k) % 5] for k in (0, 2, 4)):
            if dist == "uniform":
                d = rng.integers(0, 1 << 16, n, dtype=np.int64)
                d[rng.choice(n, 2, replace=False)] = (0, 0xFFFF)
            elif dist == "equal":       # one digit takes a whole trip in both passes
                d = np.full(n, 0xA5C3, np.int64)
            elif dist == "high-byte":   # two values that differ only in the high byte
                d = np.where(rng.random(n) < 0.5, 0x3C5A, 0xC35A).astype(np.int64)
            elif dist == "low-byte":    # ... only in the low byte
                d = np.where(rng.random(n) < 0.5, 0x5A3C, 0x5AC3).astype(np.int64)
            else:
                d = np.sort(rng.integers(0, 1 << 16, n, dtype=np.int64))[::-1].copy()
            out.append((f"global {dist} n={n}", d))
    return out


def _build_zoo():
    rng = np.random.default_rng(20240607)
    segs = _lds_segments(rng) + _order_segments(rng) + _global_segments(rng)
    return tuple((name, d.astype(np.uint32)) for name, d in segs)


ZOO = _build_zoo()   # ((name, depth16 as u32 in emission order), ...): built once, never modified
for _, _d in ZOO:
    _d.setflags(write=False)


def values_for(count, seed):
    """Distinct u32 values that are neither the index nor sorted: a seeded permutation xor a constant."""
    return (np.random.default_rng(seed).permutation(count).astype(np.uint32) ^ np.uint32(0x5A5A0000))


def place_zoo(total_tiles, seed, zoo=ZOO):
    """tile[i] for every zoo segment i, by a seeded permutation of the tile numbers -- with a fixed frame that every layout has: the first
    and the last tile empty, and one global segment directly followed by three empty tiles and then an LDS segment (segment_sort's walk to
    the next non-empty range entry).  Returns (tiles, frame) with frame = (global tile, first LDS tile behind the empty run)."""
    rng = np.random.default_rng(seed)
    if total_tiles < len(zoo) + 7:
        raise ValueError(f"{total_tiles} tiles cannot hold the {len(zoo)} segments and their empty tiles")
    i_glob = next(i for i, (n, d) in enumerate(zoo) if d.size > SEG_CAP)
    i_lds = next(i for i, (n, d) in enumerate(zoo) if 2 <= d.size <= SEG_CAP)
    p = int(rng.integers(1, total_tiles - 5))           # tiles p .. p + 4, inside 1 .. T - 2
    free = np.setdiff1d(np.arange(1, total_tiles - 1), np.arange(p, p + 5))
    rest = rng.permutation(free)[: len(zoo) - 2]
    tiles = np.empty(len(zoo), np.int64)
    tiles[[i for i in range(len(zoo)) if i not in (i_glob, i_lds)]] = rest
    tiles[i_glob], tiles[i_lds] = p, p + 4
    return tiles, (p, p + 4)


def zoo_stream(total_tiles, seed, zoo=ZOO):
    """The zoo as one stream for a grid of total_tiles tiles: (keys, values, names by tile).  The segments are interleaved by a seeded shuffle
    of the stream's emission order that keeps every segment's own emission order (which is part of the case), so that the tile passes do
    real work."""
    tiles, _ = place_zoo(total_tiles, seed, zoo)
    rng = np.random.default_rng(seed + 1)
    sizes = np.array([d.size for _, d in zoo])
    owner = rng.permutation(np.repeat(np.arange(len(zoo)), sizes))   # which segment emits at each stream position
    order = np.argsort(owner, kind="stable")                          # stream positions, segment by segment, ascending inside a segment
    keys = np.empty(owner.size, np.uint32)
    keys[order] = np.concatenate([((t + 1) << 16) | d.astype(np.int64) for t, (_, d) in zip(tiles, zoo)]).astype(np.uint32)
    names = {int(t): name for t, (name, _) in zip(tiles, zoo)}
    return keys, values_for(keys.size, seed + 2), names


def column_order(keys, values, num_tiles_x):
    """The stream as emit_scatter hands it to the row pass: stably ordered by the tile column."""
    col = ((keys >> 16).astype(np.int64) - 1) % num_tiles_x
    o = np.argsort(col, kind="stable")
    return keys[o], values[o]


def expected_sort(keys, values):
    o = np.argsort(keys, kind="stable")
    return keys[o], values[o]


def expected_ranges(sorted_keys, total_tiles):
    """ranges[t] = first index with key >> 16 == t + 1, else 0xFFFFFFFF; ranges[T] = E."""
    r = np.full(total_tiles + 1, EMPTY, np.uint32)
    tile = (sorted_keys >> 16).astype(np.int64) - 1
    if tile.size:
        first = np.flatnonzero(np.concatenate([[True], tile[1:] != tile[:-1]]))
        r[tile[first]] = first.astype(np.uint32)
    r[total_tiles] = sorted_keys.size
    return r


def expected(keys, values, total_tiles):
    k, v = expected_sort(keys, values)
    return k, v, expected_ranges(k, total_tiles)


def describe_mismatch(got_keys, ref_keys, names):
    """Which zoo segment the first differing entry belongs to (for the assertion message)."""
    bad = np.flatnonzero(got_keys != ref_keys)
    if bad.size == 0:
        return ""
    t = int(ref_keys[bad[0]] >> 16) - 1
    return f" -- first difference at index {int(bad[0])}, tile {t}: {names.get(t, 'no zoo segment')}"


_CASES = {}


def zoo_case(total_tiles, num_tiles_x=None, seed=7):
    """The zoo for a grid, with its expected result: dict(keys, values, ref_keys, ref_values, ref_ranges, names), computed once per (grid, seed)
    and shared read-only.  num_tiles_x: the stream is put into tile-column order first (the row route's input)."""
    at = (total_tiles, num_tiles_x, seed)
    if at not in _CASES:
        keys, values, names = zoo_stream(total_tiles, seed)
        if num_tiles_x:
            keys, values = column_order(keys, values, num_tiles_x)
        rk, rv, rr = expected(keys, values, total_tiles)
        for a in (keys, values, rk, rv, rr):
            a.setflags(write=False)
        _CASES[at] = dict(keys=keys, values=values, ref_keys=rk, ref_values=rv, ref_ranges=rr, names=names)
    return _CASES[at]
