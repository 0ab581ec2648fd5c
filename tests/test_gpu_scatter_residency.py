"""GPU: the tile sort's two scatter kernels at the edges of their staging -- sort_scatter_kernel (sort.hip) reorders a partition in ONE LDS
array used twice, keys first, then values through the same words; emit_scatter_kernel (project.hip) ranks its chunks the same way.  The row
pass is driven through wdgs_debug_sort_tiles on a sorter large enough to have partitions of 4096 keys (ITEMS = 16), emit_scatter through a
forward pass; keys, values and the range table are compared bit for bit with a stable numpy sort (tests/sortcases.py).  The forward pass's
unsorted stream is read from the pass itself with skipSort, which takes the plain emit kernel, not emit_scatter."""
import numpy as np
import pytest

from webdgs_amd import _lib, synth

import harness
import sortcases as sc
from harness import assert_bits_equal
from test_gpu_sort_routes import Routes, _same

pytestmark = pytest.mark.gpu

PART = sc.SORT_ITEMS_MAX * sc.SORT_THREADS   # 4096 keys per partition


@pytest.fixture(scope="module")
def rig(hip_device):
    r = Routes(hip_device, sc.SMALL_SORTER_MAX + 1, 65534)
    assert r.so.capacity > sc.SMALL_SORTER_MAX and r.so.capacity % PART == 0
    yield r
    r.destroy()


def _row_route(rig, nx, ny, tile, seed, what):
    """tile[i] in stream order -> keys with random depths, put into tile-column order (the row pass's input), through route 1."""
    rng = np.random.default_rng(seed)
    keys = (((np.asarray(tile, np.int64) + 1) << 16) | rng.integers(0, 1 << 16, len(tile))).astype(np.uint32)
    keys, vals = sc.column_order(keys, sc.values_for(keys.size, seed), nx)
    _same(rig.run(1, nx, ny, keys, vals, guard_pairs=True), *sc.expected(keys, vals, nx * ny), what)
    return keys


@pytest.mark.parametrize("count", [1, PART - 1, PART, PART + 1, 2 * PART + 1])
def test_partition_edges(rig, count):
    """One entry, one short of a partition, a full one, one more, and two full ones and one more: the last partition's bounds in both phases."""
    tile = np.random.default_rng(count).integers(0, 20 * 16, count)
    _row_route(rig, 20, 16, tile, count, f"row pass, {count} entries")


def test_one_row_fills_the_staging_array(rig):
    """Every entry in one tile row: one digit owns all 4096 words of the staging array, for the keys and again for the values."""
    nx, ny = 64, 8
    tile = 3 * nx + np.random.default_rng(3).integers(0, nx, 3 * PART + 17)
    _row_route(rig, nx, ny, tile, 3, "row pass, every entry in row 3")


def test_255_rows_of_one_entry(rig):
    """255 digits with a run of one entry each."""
    nx, ny = 2, 255
    tile = np.random.default_rng(255).permutation(ny) * nx + np.arange(ny) % nx
    _row_route(rig, nx, ny, tile, 255, "row pass, 255 rows with one entry each")


def test_tile_starts_at_element_0_of_a_partition(rig):
    """Partition 0 holds tile column 0 only, partition 1 column 1 only: tile (row 0, column 1) lies wholly in partition 1 and its first entry is
    element 0 of that partition's sorted order, where the range update has no predecessor to compare with (the `e == 0` branch)."""
    nx, ny = 4, 4
    rng = np.random.default_rng(41)
    row = np.concatenate([rng.integers(0, ny, PART), [0], rng.integers(0, ny, PART - 1)])
    col = np.repeat([0, 1], PART)
    keys = _row_route(rig, nx, ny, row * nx + col, 41, "row pass, a tile whose first entry is element 0 of partition 1")
    at = ((keys >> 16).astype(np.int64) - 1)
    assert (at[:PART] % nx == 0).all() and (at[PART:] % nx == 1).all() and (at[PART:] == 1).any(), "the stream is not what the case describes"


# ----------------------------------------------------------------------------- emit_scatter, through the forward pass
CFG = synth.SceneConfig(1, 3072, 1024, 1024, 0, 1000.0, 0.02, "scatter-residency")   # 64 x 64 tiles, twelve workgroups of emit_scatter
HIDDEN = slice(256, 512)                                                                # the Gaussians of workgroup 1, put behind the camera
ES_CHUNK = 2048


@pytest.fixture(scope="module")
def frame(hip_device):
    """The scene, its unsorted entry stream (emission order, read from a skipSort pass) and the pass's per-Gaussian tables."""
    g, sh, cam = harness.scene(CFG)
    g16 = g.view(np.uint16).reshape(-1, 12)
    g16[HIDDEN, 2] = synth.f32_to_f16_bits(np.float32(-5.0))   # z
    pipe = harness.HipPipeline(hip_device, CFG, g, sh, cam)
    try:
        pipe.fwd.encode(None, dict(skipSort=True))
        e = int(pipe.fwd.check()[0])
        r = pipe.fwd.getResources()
        keys, vals = r["tileKeysBuffer"].read(np.uint32, count=e), r["tileIndicesBuffer"].read(np.uint32, count=e)
        counts = r["tileCountsBuffer"].read(np.uint32)[:CFG.num_points].astype(np.int64)
        hip_device.synchronize()
    finally:
        pipe.destroy()
    assert e == counts.sum() and (r["numTilesX"], r["numTilesY"]) == (64, 64)
    per_wg = counts.reshape(-1, 256).sum(axis=1)
    assert per_wg[1] == 0 and counts[HIDDEN].max() == 0, "workgroup 1 was to have no entries"
    assert per_wg.max() > ES_CHUNK, f"no workgroup has a second chunk: {per_wg}"
    for a in (keys, vals, g, sh, cam):
        a.setflags(write=False)
    return dict(g=g, sh=sh, cam=cam, keys=keys, vals=vals, e=e)


def _forward(dev, frame, cap):
    pipe = harness.HipPipeline(dev, CFG, frame["g"].copy(), frame["sh"].copy(), frame["cam"], max_tile_entries=cap)
    try:
        if cap and cap < frame["e"]:
            with pytest.raises(_lib.CapacityError) as err:
                pipe.forward()
            assert f"{frame['e']} entries needed" in str(err.value), str(err.value)
            dev.synchronize()
        else:
            pipe.forward()
        assert not cap or pipe.fwd.getResources()["maxTileEntries"] == cap
        got = pipe.collect_forward()
        dev.synchronize()
    finally:
        pipe.destroy()
    return got


def test_forward_two_chunks_and_an_empty_workgroup(hip_device, frame):
    """Workgroups with more than one chunk of 2048 entries beside one whose Gaussians are all invisible (`total == 0`: it leaves before the
    first chunk): the pass's sorted list and range table are the stable sort of its own emission-order stream."""
    got = _forward(hip_device, frame, 0)
    assert got["total_entries"] == frame["e"] and got["stats"][2] == 0
    _same((got["sorted_keys"], got["sorted_values"], got["tile_ranges"]), *sc.expected(frame["keys"], frame["vals"], CFG.total_tiles), "forward pass, room for every entry")


def test_forward_capacity_cuts_the_list_inside_a_chunk(hip_device, frame):
    """Room for about half of the entries: emit_scatter writes exactly the entries whose place in tile-column order lies below the capacity --
    the cut runs through the chunks of most workgroups -- the overflow is reported with the number of entries needed, and what the pass keeps is
    the stable sort of that prefix."""
    cap = frame["e"] // 2 // PART * PART
    assert 0 < cap < frame["e"] and cap % PART == 0
    got = _forward(hip_device, frame, cap)
    assert got["total_entries"] == cap, got["stats"]
    ck, cv = sc.column_order(frame["keys"], frame["vals"], CFG.tiles_x)
    _same((got["sorted_keys"], got["sorted_values"], got["tile_ranges"]), *sc.expected(ck[:cap], cv[:cap], CFG.total_tiles), f"forward pass, room for {cap} of {frame['e']} entries")
