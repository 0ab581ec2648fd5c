"""GPU: the forward pass's tile sort routes driven directly, on crafted key streams (tests/sortcases.py), through the test hook
wdgs_debug_sort_tiles: route 0 = sorter_sort_segmented, route 1 = sorter_sort_rows, route 2 = the range search alone.  The reference is a
stable sort of the 32-bit keys and a lower-bound search for the ranges; every comparison is bit for bit -- keys, values and the whole
range table."""
import numpy as np
import pytest

from webdgs_amd import _lib, ops

import sortcases as sc
from harness import assert_bits_equal

pytestmark = pytest.mark.gpu

GUARD = 8                      # sentinel words behind the used part of a buffer
SENTINEL = 0xDEADBEEF


class Routes:
    """One sorter, its stats word and a range table, reused across the cases of a test."""

    def __init__(self, dev, capacity, max_tiles):
        self.dev = dev
        self.stats = dev.createBuffer(16)
        self.so = ops.get_dynamic_sorter(capacity, dev, self.stats)
        self.ranges = dev.createBuffer(4 * (max_tiles + 1 + GUARD))
        self.max_tiles = max_tiles

    def destroy(self):
        self.so.destroy()

    def call(self, route, nx, ny, ranges_ptr="own"):
        return self.dev.lib.wdgs_debug_sort_tiles(self.so.handle, route, nx, ny, self.ranges.ptr if ranges_ptr == "own" else ranges_ptr)

    def run(self, route, nx, ny, keys, values, guard_pairs=False, fresh_ranges=True):
        """Loads the pairs into ping-pong 0, runs the route and returns (keys, values, ranges[T + 1]) as the device left them.  The words
        behind the range table (and, guard_pairs, behind the used part of all four pair buffers) must come back untouched."""
        T, e = nx * ny, int(keys.size)
        assert T <= self.max_tiles and e + GUARD <= self.so.capacity
        pp = self.so.ping_pong
        self.stats.write(np.array([e, 0, 0, 0], np.uint32))
        if e:
            pp[0]["sort_depths_buffer"].write(keys)
            pp[0]["sort_indices_buffer"].write(values)
        guard = np.full(GUARD, SENTINEL, np.uint32)
        if guard_pairs:
            for p in pp:
                for b in p.values():
                    b.write(guard, offset=4 * e)
        if fresh_ranges:
            self.ranges.write(np.full(T + 1 + GUARD, SENTINEL, np.uint32))
        else:
            self.ranges.write(guard, offset=4 * (T + 1))
        _lib.check(self.call(route, nx, ny))
        out = pp[self.dev.lib.wdgs_sorter_final_out_index(self.so.handle)]
        assert route != 2 or out is pp[0]
        gk, gv = out["sort_depths_buffer"].read(np.uint32, count=e), out["sort_indices_buffer"].read(np.uint32, count=e)
        gr = self.ranges.read(np.uint32, count=T + 1 + GUARD)
        assert_bits_equal(gr[T + 1:], guard, f"route {route}, {nx} x {ny}: the words behind the range table")
        if guard_pairs:
            for i, p in enumerate(pp):
                for name, b in p.items():
                    assert_bits_equal(b.read(np.uint32, count=GUARD, offset=4 * e), guard, f"route {route}, {nx} x {ny}: the words behind the {e} entries of ping-pong {i} {name}")
        self.dev.synchronize()   # (lets go of the host arrays the writes were given)
        return gk, gv, gr[:T + 1]


def _same(got, ref_keys, ref_values, ref_ranges, what, names=None):
    gk, gv, gr = got
    try:
        assert_bits_equal(gk, ref_keys, what + ": sorted keys")
        assert_bits_equal(gv, ref_values, what + ": values follow a STABLE sort of the keys")
        assert_bits_equal(gr, ref_ranges, what + ": range table")
    except AssertionError as err:
        where = sc.describe_mismatch(gk, ref_keys, names or {}) if gk.shape == ref_keys.shape else ""
        if not where and gk.shape == ref_keys.shape and gv.shape == ref_values.shape:
            bad = np.flatnonzero(gv != ref_values)
            if bad.size:
                t = int(ref_keys[bad[0]] >> 16) - 1
                where = f" -- first value out of order at index {int(bad[0])}, tile {t}: {(names or {}).get(t, 'no zoo segment')}"
        raise AssertionError(str(err) + where) from None


def _zoo(rig, route, nx, ny, **kw):
    case = sc.zoo_case(nx * ny, nx if route == 1 else None)
    got = rig.run(route, nx, ny, case["keys"], case["values"], guard_pairs=True, **kw)
    _same(got, case["ref_keys"], case["ref_values"], case["ref_ranges"], f"zoo through route {route}, {nx} x {ny} tiles", case["names"])
    return got


ZOO_ENTRIES = sum(d.size for _, d in sc.ZOO)


def test_zoo_through_the_tile_bit_passes(hip_device):
    """Route 0: 255 tiles = one tile pass and the range table from tile_ranges_kernel; 256 = the first two-pass grid (4 + 5 bits, the
    scatter builds the table); 8191 / 8192 = 13 / 14 bits; 65534 = 8 + 8 bits."""
    rig = Routes(hip_device, ZOO_ENTRIES + 5000, 65534)
    try:
        for T in (255, 256, 8191, 8192, 65534):
            _zoo(rig, 0, T, 1)
    finally:
        rig.destroy()


@pytest.mark.parametrize("T", [1, 2, 7, 8])
def test_tiny_grids_through_the_tile_bit_passes(hip_device, T):
    """A few hundred entries over every tile but one (T = 1: all in the single tile), in both arrangements of the grid."""
    rng = np.random.default_rng(100 + T)
    rig = Routes(hip_device, 5000, T)
    try:
        for empty in ([None] if T == 1 else [0, T // 2, T - 1]):
            live = np.array([t for t in range(T) if t != empty])
            tile = np.concatenate([live, rng.choice(live, 700 - live.size)])
            rng.shuffle(tile)
            keys = (((tile + 1) << 16) | rng.integers(0, 1 << 16, tile.size)).astype(np.uint32)
            vals = sc.values_for(keys.size, T)
            for nx, ny in {(T, 1), (1, T)}:
                _same(rig.run(0, nx, ny, keys, vals, guard_pairs=True), *sc.expected(keys, vals, T), f"{nx} x {ny} tiles, tile {empty} empty")
    finally:
        rig.destroy()


def test_zoo_through_the_row_pass(hip_device):
    """Route 1 on the zoo in tile-column order: the reciprocal row digit, the atomicMin range table, and segment_sort behind them."""
    rig = Routes(hip_device, ZOO_ENTRIES + 5000, 65534)
    try:
        for nx, ny in ((20, 16), (256, 255), (2, 256), (251, 256)):
            _zoo(rig, 1, nx, ny)
    finally:
        rig.destroy()


def _column_sweep(dev, shapes):
    rig = Routes(dev, 65534 * 5 // 4 + 5000, 65534)
    try:
        for i, (nx, ny) in enumerate(shapes):
            T = nx * ny
            rng = np.random.default_rng(1000 * nx + ny)
            tile = np.concatenate([np.arange(T), rng.integers(0, T, T // 4)])
            if i % 4 == 3:   # a random tenth of the tiles emptied
                gone = np.zeros(T, bool)
                gone[rng.choice(T, max(T // 10, 1), replace=False)] = True
                tile = tile[~gone[tile]]
            tile = rng.permutation(tile)
            keys = (((tile + 1) << 16) | rng.integers(0, 1 << 16, tile.size)).astype(np.uint32)
            keys, vals = sc.column_order(keys, sc.values_for(keys.size, nx), nx)
            _same(rig.run(1, nx, ny, keys, vals), *sc.expected(keys, vals, T), f"row pass, {nx} x {ny} tiles")
    finally:
        rig.destroy()


def test_row_digit_at_every_column_count(hip_device):
    """sort.hip's DigitOf says of its reciprocal multiply "exact: tile < 2^16, num_tiles_x <= 256": every num_tiles_x in 2..256 with the
    tallest grid the forward pass can have, every tile populated (on every fourth shape a random tenth emptied), and the one-row grids
    (dmask = 0)."""
    _column_sweep(hip_device, [(nx, min(256, 65534 // nx)) for nx in range(2, 257)] + [(2, 1), (3, 1), (256, 1)])


ROUTE2_COUNTS = (0, 1, 2, 64, 65, 66, 4224, 4225, 4226, 274_625, 274_626, 1_000_003)   # 64, 65^2, 65^3: where the 64-ary search takes one more round
ROUTE2_TILES = (1, 3, 64, 300, 65534)


def _random_tiles(rng, count, T):
    alive = np.ones(T, bool)
    for _ in range(int(rng.integers(1, 6))):   # runs of empty tiles
        a = int(rng.integers(0, T))
        alive[a:a + int(rng.integers(1, max(2, T // 3)))] = False
    if not alive.any():
        alive[int(rng.integers(0, T))] = True
    return np.sort(rng.choice(np.flatnonzero(alive), count))


def test_range_search_alone(hip_device):
    """Route 2: tile_ranges_kernel on host-sorted keys -- counts around the powers of 65 at which the search takes another round, grids
    from one tile to 65534, all entries in one tile / one entry per tile / random with runs of empty tiles; then 200 random pairs."""
    rng = np.random.default_rng(65)
    rig = Routes(hip_device, max(ROUTE2_COUNTS) + 5000, 65534)
    turn = 0
    try:
        cases = [(c, T, d) for c in ROUTE2_COUNTS for T in ROUTE2_TILES for d in ("one-tile", "one-per-tile", "random")]
        cases += [(int(rng.integers(0, 5001)), int(rng.integers(1, 401)), "random") for _ in range(200)]
        for count, T, dist in cases:
            if dist == "one-tile":
                tile = np.full(count, (0, T // 2, T - 1)[turn % 3])
                turn += 1
            elif dist == "one-per-tile":   # as far as the count reaches; what is left over goes to the last tile
                tile = np.minimum(np.arange(count), T - 1)
            else:
                tile = _random_tiles(rng, count, T)
            keys = np.sort((((tile + 1) << 16) | rng.integers(0, 1 << 16, count)).astype(np.uint32))
            vals = sc.values_for(count, count & 0xFFFF)
            ref = sc.expected_ranges(keys, T)
            _same(rig.run(2, T, 1, keys, vals), keys, vals, ref, f"range search, {count} entries, {T} tiles, {dist}")
    finally:
        rig.destroy()


def test_empty_list_through_every_route(hip_device):
    """E = 0: every tile empty, ranges[T] = 0, and nothing written behind the (empty) used part of the pair buffers."""
    rig = Routes(hip_device, 5000, 65534)
    none = np.zeros(0, np.uint32)
    try:
        for route, nx, ny in ((0, 255, 1), (0, 256, 1), (0, 65534, 1), (0, 1, 1), (1, 20, 16), (1, 256, 255), (1, 2, 1), (2, 300, 1), (2, 65534, 1), (2, 1, 1)):
            T = nx * ny
            _, _, gr = rig.run(route, nx, ny, none, none, guard_pairs=True)
            assert_bits_equal(gr, np.concatenate([np.full(T, sc.EMPTY, np.uint32), np.zeros(1, np.uint32)]), f"route {route}, {nx} x {ny}: range table of an empty list")
    finally:
        rig.destroy()


def test_argument_checks(hip_device):
    """What the forward pass can never ask for is refused with WDGS_E_INVALID, and a valid call afterwards still works."""
    rig = Routes(hip_device, 5000, 65534)
    try:
        refused = [("unknown route", lambda: rig.call(3, 4, 4)),
                   ("no tiles (0 x 5)", lambda: rig.call(0, 0, 5)), ("no tiles (5 x 0)", lambda: rig.call(0, 5, 0)),
                   ("65535 tiles", lambda: rig.call(0, 65535, 1)), ("256 x 256 tiles", lambda: rig.call(1, 256, 256)),
                   ("65536 x 65536 tiles", lambda: rig.call(0, 65536, 65536)), ("65535 tiles, range search", lambda: rig.call(2, 1, 65535)),
                   ("null range table", lambda: rig.call(0, 4, 4, None)), ("null range table, range search", lambda: rig.call(2, 4, 4, None)),
                   ("null sorter", lambda: hip_device.lib.wdgs_debug_sort_tiles(None, 0, 4, 4, rig.ranges.ptr)),
                   ("row route, one column", lambda: rig.call(1, 1, 16)), ("row route, 257 columns", lambda: rig.call(1, 257, 2)),
                   ("row route, 257 rows", lambda: rig.call(1, 2, 257))]
        for what, call in refused:
            code = call()
            assert code == _lib.WDGS_E_INVALID, f"{what}: returned {code}"
            with pytest.raises(_lib.WdgsError) as err:
                _lib.check(code)
            assert err.value.code == _lib.WDGS_E_INVALID and "wdgs_debug_sort_tiles" in str(err.value), what
        rng = np.random.default_rng(9)
        keys = (((rng.integers(0, 16, 500) + 1) << 16) | rng.integers(0, 1 << 16, 500)).astype(np.uint32)
        vals = sc.values_for(500, 9)
        _same(rig.run(0, 4, 4, keys, vals), *sc.expected(keys, vals, 16), "a valid call after the refusals")
        ck, cv = sc.column_order(keys, vals, 4)
        _same(rig.run(1, 4, 4, ck, cv), *sc.expected(ck, cv, 16), "a valid row-route call after the refusals")
    finally:
        rig.destroy()


def test_a_sorter_keeps_nothing_from_its_last_sort(hip_device):
    """The zoo through route 1 twice on one sorter and one range table, with differently shaped sorts in between (whose table and counts
    stay in the buffers): the second result equals the first bit for bit."""
    rig = Routes(hip_device, ZOO_ENTRIES + 5000, 65534)
    try:
        first = _zoo(rig, 1, 256, 255)
        _zoo(rig, 1, 20, 16, fresh_ranges=False)
        _zoo(rig, 0, 8191, 1, fresh_ranges=False)
        second = _zoo(rig, 1, 256, 255, fresh_ranges=False)
        for a, b, what in zip(first, second, ("keys", "values", "range table")):
            assert_bits_equal(b, a, f"second run of the same sort: {what}")
    finally:
        rig.destroy()
