"""CPU: the crafted key streams of tests/sortcases.py are what tests/test_gpu_sort_routes.py believes they are -- written for the constants
sort.hip has today, covering every per-tile branch of segment_sort from both sides of every edge, with a reference that a second,
differently written one confirms.  No GPU and no library."""
import os
import re

import numpy as np

import sortcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_HIP = open(os.path.join(ROOT, "webdgs_amd", "csrc", "sort.hip")).read()


def _constant(name):
    m = re.search(r"constexpr\s+u32\s+" + name + r"\s*=\s*(\d+)\s*;", SORT_HIP)
    assert m, f"sort.hip no longer defines `constexpr u32 {name} = <number>;`: tests/sortcases.py was written for it"
    return int(m.group(1))


def test_the_zoo_was_written_for_the_constants_sort_hip_has():
    moved = "tests/sortcases.py places its edges by this constant: move them with it"
    assert _constant("SEG_CAP") == sc.SEG_CAP, moved
    assert _constant("SEG_WIDE_BITS") == sc.SEG_WIDE_BITS, moved
    assert _constant("SORT_ITEMS_MAX") == sc.SORT_ITEMS_MAX, moved
    assert _constant("SORT_THREADS") == sc.SORT_THREADS, moved
    m = re.search(r"s->items\s*=\s*s->capacity\s*<=\s*\((\d+)u\s*<<\s*(\d+)\)\s*\?\s*(\d+)u\s*:\s*SORT_ITEMS_MAX", SORT_HIP)
    assert m, "sort.hip no longer chooses a sorter's partition size by `s->capacity <= (8u << 20) ? 4u : SORT_ITEMS_MAX`"
    assert int(m.group(1)) << int(m.group(2)) == sc.SMALL_SORTER_MAX and int(m.group(3)) == sc.SORT_ITEMS_SMALL, moved
    # the span tests of segment_sort_kernel, in the order classify() applies them
    assert re.search(r"hi16 - lo16 < \(1u << 8\)", SORT_HIP) and re.search(r"hi16 - lo16 < \(1u << 9\)", SORT_HIP) and re.search(r"hi16 - lo16 < SEG_BINS", SORT_HIP), moved
    assert re.search(r"if \(n <= SEG_CAP\)", SORT_HIP), moved
    assert re.search(r"base < active; base \+= 1024u", SORT_HIP) and sc.SCAN_ROWS_STEP == 1024, moved
    assert re.search(r"c0 < n; c0 \+= 4u \* SEG_THREADS", SORT_HIP) and _constant("SEG_THREADS") * 4 == sc.GLOBAL_TRIP, moved


def _segments():
    return [(name, d, int(d.size), int(d.max()) - int(d.min())) for name, d in sc.ZOO]


def test_zoo_holds_the_lengths_spans_and_patterns():
    segs = _segments()
    assert len({name for name, *_ in segs}) == len(segs), "segment names are unique"
    assert len(segs) < 255 - 7, "the whole zoo fits a grid of 255 tiles, with its empty tiles"
    total = sum(n for _, _, n, _ in segs)
    assert 150_000 <= total <= 250_000, total
    lds = {(n, span) for name, d, n, span in segs if name.startswith("lds ")}
    assert lds == {(n, s) for n in sc.LDS_LENGTHS for s in sc.LDS_SPANS if s == 0 or n >= 2}
    for name, d, n, span in segs:
        assert d.dtype == np.uint32 and n >= 1 and d.max() <= 0xFFFF
        if name.startswith("global "):
            assert n > sc.SEG_CAP
    assert {n for name, d, n, span in segs if name.startswith("global ")} == set(sc.GLOBAL_LENGTHS)
    assert {name.split()[1] for name, *_ in segs if name.startswith("global ")} == set(sc.GLOBAL_DISTRIBUTIONS)
    assert any(n % sc.GLOBAL_TRIP == 0 for name, d, n, span in segs if name.startswith("global ")), "a length that is a multiple of the trip"
    # the wave split per_wave = roundup64(ceil(n / 4)) changes at 256 / 257
    assert {255, 256, 257} <= {n for _, _, n, _ in segs}
    # the minimum rotates over bottom, top and across a bin multiple
    mins = {int(d.min()) for name, d, n, span in segs if name.startswith("lds ") and span == 255}
    assert 0 in mins and 0xFFFF - 255 in mins and len(mins) >= 3
    # order patterns: four per (length, LDS branch)
    for n in sc.ORDER_LENGTHS:
        for span in sc.ORDER_SPANS:
            kinds = {name.split()[1] for name, d, m, s in segs if name.startswith("order ") and m == n and s == span}
            assert kinds == {"ascending", "descending", "two-values", "all-equal-but-last"}, (n, span, kinds)
    assert {sc.classify(300, s) for s in sc.ORDER_SPANS} == set(sc.BRANCHES) - {"global"}
    for name, d, n, span in segs:
        if " ascending " in name:
            assert (np.diff(d.astype(np.int64)) >= 0).all()
        if " descending " in name or name.startswith("global descending"):
            assert (np.diff(d.astype(np.int64)) <= 0).all()
        if " two-values " in name:
            assert np.unique(d).size == 2
        if " all-equal-but-last " in name:
            assert np.unique(d[:-1]).size == 1 and d[-1] < d[0]


def test_every_branch_and_every_edge_is_hit_from_both_sides():
    segs = _segments()
    by_branch = {b: [(name, d, n, span) for name, d, n, span in segs if sc.classify(n, span) == b] for b in sc.BRANCHES}
    for b in sc.BRANCHES:
        assert by_branch[b], f"no zoo segment takes the {b} branch"
    lds_spans = {span for _, _, n, span in segs if n <= sc.SEG_CAP and n >= 2}
    for edge in (1 << 8, 1 << 9, 1 << sc.SEG_WIDE_BITS):
        assert edge - 1 in lds_spans and edge in lds_spans, f"span {edge - 1} / {edge}"
        assert sc.classify(2, edge - 1) != sc.classify(2, edge)
    lengths = {n for _, _, n, _ in segs}
    assert sc.SEG_CAP in lengths and sc.SEG_CAP + 1 in lengths
    assert sc.classify(sc.SEG_CAP, 0) != "global" and sc.classify(sc.SEG_CAP + 1, 0) == "global"
    # every one-pass branch: a segment that a digit of the RAW low depth bits misorders, while the digit of depth - min sorts it
    for b, bits in sc.ONE_PASS_BITS.items():
        wraps = []
        for name, d, n, span in by_branch[b]:
            di = d.astype(np.int64)
            right = np.argsort(di, kind="stable")
            assert np.array_equal(np.argsort((di - di.min()) & ((1 << bits) - 1), kind="stable"), right), name
            if not np.array_equal(np.argsort(di & ((1 << bits) - 1), kind="stable"), right):
                wraps.append(name)
        assert wraps, f"no {b} segment lies across a multiple of {1 << bits}"
    # every span edge: taking the narrower route for the span AT the edge misorders the segment (what `<=` for `<` would do)
    for bits in (8, 9, sc.SEG_WIDE_BITS):
        hit = False
        for name, d, n, span in segs:
            if n <= sc.SEG_CAP and span == 1 << bits:
                di = d.astype(np.int64)
                hit |= not np.array_equal(np.argsort((di - di.min()) & ((1 << bits) - 1), kind="stable"), np.argsort(di, kind="stable"))
        assert hit, f"span {1 << bits}"


def test_layouts_hold_the_empty_tiles():
    for T in (255, 256, 8191, 8192, 65534):
        tiles, (glob, lds) = sc.place_zoo(T, 5)
        assert np.unique(tiles).size == len(sc.ZOO) and tiles.min() >= 1 and tiles.max() <= T - 2, "first and last tile empty"
        used = set(tiles.tolist())
        assert glob in used and lds == glob + 4 and lds in used and not {glob + 1, glob + 2, glob + 3} & used
        size = {int(t): d.size for t, (_, d) in zip(tiles, sc.ZOO)}
        assert size[glob] > sc.SEG_CAP and 2 <= size[lds] <= sc.SEG_CAP
    a, b = sc.place_zoo(8192, 5)[0], sc.place_zoo(8192, 6)[0]
    assert not np.array_equal(a, b) and np.array_equal(a, sc.place_zoo(8192, 5)[0]), "seeded"


def _reference_two(keys, values, total_tiles):
    """The same result written differently: a lexicographic sort on (tile, depth16, position), a binary search for the ranges."""
    tile, depth = (keys >> 16).astype(np.int64), (keys & 0xFFFF).astype(np.int64)
    o = np.lexsort((np.arange(keys.size), depth, tile))
    k = keys[o]
    want = np.arange(1, total_tiles + 1)
    lo = np.searchsorted(k >> 16, want, side="left")
    hi = np.searchsorted(k >> 16, want, side="right")
    r = np.where(hi > lo, lo, sc.EMPTY).astype(np.uint32)
    return k, values[o], np.concatenate([r, [keys.size]]).astype(np.uint32)


def test_reference_agrees_with_a_second_one():
    for T, nx in ((255, None), (8192, None), (256 * 255, 256), (20 * 16, 20)):
        keys, vals, names = sc.zoo_stream(T, 3)
        assert keys.size == sum(d.size for _, d in sc.ZOO) and np.unique(vals).size == vals.size
        assert not np.array_equal(vals, np.arange(vals.size)) and (np.diff(vals.astype(np.int64)) < 0).any()
        tile = (keys >> 16).astype(np.int64) - 1
        assert tile.min() >= 1 and tile.max() <= T - 2
        assert (np.diff(tile) != 0).mean() > 0.9, "the stream is interleaved: the tile passes have work to do"
        for t, (name, d) in zip(sc.place_zoo(T, 3)[0], sc.ZOO):   # every segment keeps its emission order
            assert names[int(t)] == name
            if d.size in (300, 2049):
                assert np.array_equal(keys[tile == t] & 0xFFFF, d)
        if nx:
            keys, vals = sc.column_order(keys, vals, nx)
            col = ((keys >> 16).astype(np.int64) - 1) % nx
            assert (np.diff(col) >= 0).all()
        k, v, r = sc.expected(keys, vals, T)
        k2, v2, r2 = _reference_two(keys, vals, T)
        assert np.array_equal(k, k2) and np.array_equal(v, v2) and np.array_equal(r, r2)
        assert r[0] == sc.EMPTY and r[T - 1] == sc.EMPTY and r[T] == keys.size
    # small hand-made cases, the empty list among them
    k, v, r = sc.expected(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3)
    assert k.size == 0 and r.tolist() == [sc.EMPTY] * 3 + [0]
    keys = np.array([(3 << 16) | 5, (1 << 16) | 9, (3 << 16) | 5, (1 << 16) | 2], np.uint32)
    k, v, r = sc.expected(keys, np.array([10, 11, 12, 13], np.uint32), 4)
    assert v.tolist() == [13, 11, 10, 12] and r.tolist() == [0, sc.EMPTY, 2, sc.EMPTY, 4]
