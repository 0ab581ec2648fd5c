"""GPU: the densify kernels (csrc/densify.hip) on the crafted images, lists and tables of tests/densifycases.py, with no render in front of
them: the bilinear down-sample, the metric map, the per-Gaussian metric count, normalize, decide, cap / scans / total and the fused rebuild
scatter.  Every comparison is bit for bit against the oracle (tests/test_densify_cases.py holds the oracle itself to the plain forms on the same
inputs); the one allowance is that a NaN equals a NaN of any sign and payload, per f32 lane and per fp16 half.  Output buffers are pre-filled
with a sentinel word, and every slot the plain form says is not written must still hold it."""
import types

import numpy as np
import pytest

from webdgs_amd import ops

import densifycases as dc
from harness import assert_bits_equal, assert_f32_equal, assert_halves_equal

pytestmark = pytest.mark.gpu

SENTINEL = dc.SENTINEL
KEYS = tuple(dc.STATE_WIDTHS)
FIELD = dict(opt_pos="optPosBuffer", opt_rot="optRotBuffer", opt_scale="optScaleBuffer", opt_opacity="optOpacityBuffer", param_sh="paramSH", state_sh="stateSH")
GUARD_ROWS = 3      # sentinel rows behind every output array


# ----------------------------------------------------------------------------------------------------------------- K31
@pytest.mark.parametrize("shape", dc.DOWNSAMPLE_SHAPES, ids=dc.downsample_id)
def test_downsample_equals_the_oracle(hip_device, orc, shape):
    dev, ((sw, sh), (dw, dh)) = hip_device, shape
    src = dc.downsample_source(shape)
    dst = dev.bufferFrom(np.full(dw * dh + 64, SENTINEL, np.uint32))
    source = dev.bufferFrom(src)
    ops.downsampleRGBA8(dev, source, sw, sh, dst, dw, dh)
    got = dst.read(np.uint32)
    assert_bits_equal(got[:dw * dh].view(np.uint8).reshape(dh, dw, 4), orc.downsample_bilinear(src, dw, dh), f"down-sample {dc.downsample_id(shape)}")
    assert np.all(got[dw * dh:] == SENTINEL), "words behind the destination's last texel"


# ----------------------------------------------------------------------------------------------------------------- K21-K23
@pytest.fixture(scope="module")
def one_point_pass(hip_device):
    pc = ops.createPointCloud(hip_device, np.zeros((1, 6), np.uint32), np.zeros((1, 24), np.uint32), 3)
    mp = ops.TiledBackwardPass(hip_device, pc, dict(viewportWidth=16, viewportHeight=16, trainingConfig={}))
    yield mp
    mp.destroy()


@pytest.mark.parametrize("size", dc.METRIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_metric_map_equals_the_oracle(hip_device, orc, one_point_pass, size):
    dev, mp, (w, h) = hip_device, one_point_pass, size
    mp.setViewport(w, h)
    for kind in dc.METRIC_CONTENTS:
        pred, targ = dc.metric_images(kind, w, h)
        bp, bt = dev.bufferFrom(pred), dev.bufferFrom(targ)
        for thr in dc.METRIC_THRESHOLDS:
            mp.getMetricMapTextureView().write(np.full(w * h, SENTINEL, np.uint32))
            mp.getMetricMinMaxBuffer().write(np.full(2, SENTINEL, np.uint32))
            mp.computeMetricMap(None, bp, bt, dict(threshold=thr))
            _, mm, flags = orc.metric_map(pred, targ, thr)
            assert_bits_equal(mp.getMetricMinMaxBuffer().read(np.uint32), mm, f"{kind} {w}x{h} t={thr}: min / max")
            assert_bits_equal(mp.getMetricMapTextureView().read(np.uint32).reshape(h, w), flags, f"{kind} {w}x{h} t={thr}: flags")


# ----------------------------------------------------------------------------------------------------------------- K24
@pytest.mark.parametrize("viewport", dc.COUNT_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_metric_count_equals_the_per_pixel_form(hip_device, orc, viewport):
    """Splat records, tile ranges, lists, n_contrib and flags all written here.  The list buffer handed over ends at num_instances; the
    entries behind it exist in memory (this test's own) and would count if the walk did not stop."""
    dev, (W, H) = hip_device, viewport
    case = dc.count_case(W, H)
    n, E = case["n"], case["num_instances"]
    pc = ops.createPointCloud(dev, np.zeros((n, 6), np.uint32), np.zeros((n, 24), np.uint32), 3)
    mp = ops.TiledBackwardPass(dev, pc, dict(viewportWidth=W, viewportHeight=H, trainingConfig={}))
    try:
        lists = dev.bufferFrom(case["instances"])
        res = dict(splatBuffer=dev.bufferFrom(case["splats"]), tileOffsetsBuffer=dev.bufferFrom(case["ranges"]), tileIndicesBuffer=dev.view(lists.ptr, 4 * E),
                   nContribTexture=dev.bufferFrom(case["n_contrib"]))
        named = np.zeros(n, bool)
        ids = case["instances"][:E]
        named[ids[ids < n]] = True
        assert not named.all()
        for kind in dc.COUNT_FLAGS:
            if kind == "from-metric-map":
                pred, targ = dc.count_map_images(W, H)
                bp, bt = dev.bufferFrom(pred), dev.bufferFrom(targ)
                mp.computeMetricMap(None, bp, bt, dict(threshold=0.37))
                flags = orc.metric_map(pred, targ, 0.37)[2]
                assert_bits_equal(mp.getMetricMapTextureView().read(np.uint32).reshape(H, W), flags, f"{W}x{H}: the metric map the count reads")
            else:
                flags = dc.count_flags(kind, W, H)
                mp.getMetricMapTextureView().write(flags)
            for clear in (False, True):
                pre = dc.count_prefill(n, clear)
                mp.getMetricCountsBuffer().write(pre)
                mp.computeMetricCounts(None, res, dict(clear=clear))
                want = np.zeros(n, np.uint32) if clear else pre.copy()
                orc.metric_count(case["settings"], case["ranges"], case["instances"], E, case["splats"], flags, case["n_contrib"], want)
                got = mp.getMetricCountsBuffer().read(np.uint32)[:n]
                assert_bits_equal(got, want, f"{W}x{H} flags {kind} clear={clear}: counts")
                if not clear:
                    assert_bits_equal(got[~named], pre[~named], f"{W}x{H} flags {kind}: counts of Gaussians no list names")
                if kind == "all":
                    assert np.any(want != (0 if clear else pre))
    finally:
        mp.destroy()


# ----------------------------------------------------------------------------------------------------------------- K25
@pytest.mark.parametrize("n", dc.NORMALIZE_SIZES)
def test_normalize_equals_the_oracle(hip_device, orc, n):
    dev = hip_device
    pc = ops.createPointCloud(dev, np.zeros((n, 6), np.uint32), np.zeros((n, 24), np.uint32), 3)
    mp = ops.TiledBackwardPass(dev, pc, dict(viewportWidth=16, viewportHeight=16, trainingConfig={}))
    try:
        for d in dc.NORMALIZE_DIVISORS:
            want = dc.normalize_counts(n)
            mp.getMetricCountsBuffer().write(want)
            mp.normalizeMetricCounts(None, dict(divisor=d))
            orc.metric_normalize(want, d)
            assert_bits_equal(mp.getMetricCountsBuffer().read(np.uint32)[:n], want, f"n={n} divisor {d:#x}")
    finally:
        mp.destroy()


# ----------------------------------------------------------------------------------------------------------------- K26
def _decision(dev, orc, dp, pc, g, counts, clone, prune, split, what):
    pc.gaussian_3d_buffer.write(g)
    dp.setConfig(dict(cloneThreshold=clone, pruneThreshold=prune, splitThreshold=split))
    dp.ensureSize(pc.num_points)
    dp.getActionBuffer().write(np.full(pc.num_points, SENTINEL, np.uint32))
    dp.getOutCountBuffer().write(np.full(pc.num_points, SENTINEL, np.uint32))
    mcb = None if counts is None else dev.bufferFrom(counts)
    out = dp.encodeDecision(None, dict(pointCloud=pc, metricCountsBuffer=mcb))
    want = orc.densify_prepare(g, counts, 0xFFFFFFFF, clone_threshold=clone, prune_opacity=prune, split_scale=split)      # (a cap that never binds)
    assert_bits_equal(out["actionBuffer"].read(np.uint32), want["actions"], f"{what}: actions")
    assert_bits_equal(out["outCountBuffer"].read(np.uint32), want["counts"], f"{what}: counts")


@pytest.fixture(scope="module")
def sweep_rig(hip_device):
    n = 65536
    pc = ops.createPointCloud(hip_device, np.zeros((n, 6), np.uint32), np.zeros((n, 24), np.uint32), 3)
    dp = ops.DensifyPrunePass(hip_device, dict(strategy="gpu_rebuild", maxBufferBytes=0))
    yield pc, dp
    dp.destroy()


def test_decide_over_every_fp16_opacity(hip_device, orc, sweep_rig):
    pc, dp = sweep_rig
    g, mc = dc.decide_opacity_sweep()
    t = dc.DECIDE_CLONE_THRESHOLD
    for prune in dc.DECIDE_PRUNE_THRESHOLDS:
        for clone, counts in ((t, mc), (0, mc), (t, None), (0, None)):
            _decision(hip_device, orc, dp, pc, g, counts, clone, prune, 1.0, f"opacity sweep, prune {prune}, clone {clone}, counts {'given' if counts is not None else 'none'}")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_decide_over_every_fp16_scale(hip_device, orc, sweep_rig, axis):
    pc, dp = sweep_rig
    g, mc = dc.decide_scale_sweep(axis)
    for split in dc.DECIDE_SPLIT_THRESHOLDS:
        _decision(hip_device, orc, dp, pc, g, mc, dc.DECIDE_CLONE_THRESHOLD, 0.15, split, f"scale sweep axis {axis}, split {split}")


# ----------------------------------------------------------------------------------------------------------------- K27-K28
def _check_prepared(dp, bufs, want, n, what):
    assert_bits_equal(bufs["actionBuffer"].read(np.uint32)[:n], want["actions"], f"{what}: actions")
    assert_bits_equal(bufs["outCountBuffer"].read(np.uint32)[:n], want["counts"], f"{what}: counts")
    assert_bits_equal(bufs["outOffsetBuffer"].read(np.uint32)[:n], want["offsets"], f"{what}: offsets")
    assert dp.readTotal() == want["total"], f"{what}: total {dp.readTotal()} vs {want['total']}"


@pytest.mark.parametrize("n", dc.CAP_SIZES)
def test_cap_scans_and_total_equal_the_oracle(hip_device, orc, n):
    dev = hip_device
    g, mc, _ = dc.cap_cloud(n)
    pc = ops.createPointCloud(dev, g, np.zeros((n, 24), np.uint32), 3)
    rule = dict(cloneThreshold=6, pruneThreshold=0.15, splitThreshold=0.05)
    orule = dict(clone_threshold=6, prune_opacity=0.15, split_scale=0.05)
    dp = ops.DensifyPrunePass(dev, dict(strategy="gpu_rebuild", maxBufferBytes=0, **rule))
    try:
        mcb = dev.bufferFrom(mc)
        decided = orc.densify_prepare(g, mc, 0xFFFFFFFF, **orule)["counts"]
        dp.ensureSize(n)
        for name, max_out in dc.cap_values(decided).items():        # the staged calls, as a host sequences them itself
            dp.getOutTotalBuffer().write(np.array([SENTINEL], np.uint32))
            d = dp.encodeDecision(None, dict(pointCloud=pc, metricCountsBuffer=mcb))
            off = dp.encodePrefixSum(None)
            dp.encodeCapToMax(None, off, max_out)
            off = dp.encodePrefixSum(None)
            dp.encodeTotalOut(None, off)
            _check_prepared(dp, dict(d, outOffsetBuffer=off), orc.densify_prepare(g, mc, max_out, **orule), n, f"n={n} staged, maxOutPoints {name} = {max_out}")
        for max_bytes, new_points in ((0, 0), (9600, 0), (0, 1), (0, 40), (9600, 1), (9600, 40)):
            dp.setConfig(dict(maxBufferBytes=max_bytes, maxNewPointsPerStep=new_points))
            m = dp.computeMaxOutPoints(pc)
            assert m == dc.max_out_plain(n, max_bytes, new_points), (n, max_bytes, new_points, m)
            assert dp.computeMaxOutPoints(types.SimpleNamespace(num_points=0)) == dc.max_out_plain(0, max_bytes, new_points)
            prep = dp.encodePrepare(None, dict(pointCloud=pc, metricCountsBuffer=mcb))
            assert prep["maxOutPoints"] == m
            _check_prepared(dp, prep, orc.densify_prepare(g, mc, m, **orule), n, f"n={n} encodePrepare, {max_bytes} bytes, {new_points} new points")
    finally:
        dp.destroy()


# ----------------------------------------------------------------------------------------------------------------- K29 + K30
def _sentinel_rows(rows, width):
    return np.full((rows + GUARD_ROWS, width), SENTINEL, np.uint32)


def run_scatter(dev, orc, g, sh, st, tables, reset, with_state, what):
    """One scatter with tables written from here -- ensureSize, then the count, action and offset buffers -- into sentinel-filled outputs
    of out_n + GUARD_ROWS rows; written slots against the oracle, every other slot against the sentinel."""
    counts, actions, offsets, out_n = tables
    n = g.shape[0]
    pc = ops.createPointCloud(dev, g, sh, 3)
    dp = ops.DensifyPrunePass(dev, dict(strategy="gpu_rebuild"))
    try:
        dp.ensureSize(n)
        offb = dp.encodePrefixSum(None)
        dp.getOutCountBuffer().write(counts)
        dp.getActionBuffer().write(actions)
        offb.write(offsets)
        out_pc = ops.PointCloud("full", out_n, 3, dev.bufferFrom(_sentinel_rows(out_n, 6)), dev.bufferFrom(_sentinel_rows(out_n, 24)))
        inputs = dict(pointCloud=pc, outOffsetBuffer=offb, outNumPoints=out_n, resetNewOptimizerState=reset)
        outputs = dict(outPointCloud=out_pc)
        if with_state:
            inputs["optimizerState"] = {FIELD[k]: dev.bufferFrom(st[k]) for k in KEYS}
            outputs["outOptimizerState"] = {FIELD[k]: dev.bufferFrom(_sentinel_rows(out_n, w)) for k, w in dc.STATE_WIDTHS.items()}
        dp.encodeScatter(None, inputs, outputs)
        dev.synchronize()
        og, osh, ost = orc.densify_scatter(g, sh, st, dict(offsets=offsets, counts=counts, actions=actions), out_n, reset)
        dst, _, _ = dc.scatter_plan(counts, offsets, out_n)

        def expected(rows, width):
            want = _sentinel_rows(out_n, width)
            want[dst] = np.ascontiguousarray(rows).view(np.uint32)[dst]
            return want
        got_g = out_pc.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6)
        assert_halves_equal(dc.halves(got_g), dc.halves(expected(og, 6)), f"{what}: Gaussian words")
        assert_bits_equal(out_pc.sh_buffer.read(np.uint32).reshape(-1, 24), expected(osh, 24), f"{what}: SH rows")
        if with_state:
            for k, w in dc.STATE_WIDTHS.items():
                got = outputs["outOptimizerState"][FIELD[k]].read(np.float32).reshape(-1, w)
                assert_f32_equal(got, expected(ost[k], w).view(np.float32), f"{what}: {k}")
    finally:
        dp.destroy()


MODES = (("reset", True, True), ("carry", False, True), ("no-state", True, False))


@pytest.mark.parametrize("name,n", dc.SCATTER_CASES, ids=[f"{k}-{n}" for k, n in dc.SCATTER_CASES])
def test_scatter_tables(hip_device, orc, name, n):
    g, sh, st = dc.scatter_cloud(n)
    tables = dc.scatter_tables(name, n)
    for mode, reset, with_state in MODES:
        run_scatter(hip_device, orc, g, sh, st, tables, reset, with_state, f"{name} n={n} {mode}")


@pytest.mark.parametrize("what", ["keep", "clone", "split"])
def test_scatter_value_edges(hip_device, orc, what):
    g, sh, st = dc.value_cloud()
    for mode, reset, with_state in MODES[:2]:
        run_scatter(hip_device, orc, g, sh, st, dc.value_tables(g.shape[0], what), reset, with_state, f"value edges, {what}, {mode}")


@pytest.mark.parametrize("what", ["keep", "split"])
def test_scatter_over_every_fp16_opacity(hip_device, orc, what):
    g, sh, st = dc.opacity_sweep_cloud()
    run_scatter(hip_device, orc, g, sh, st, dc.value_tables(g.shape[0], what), True, True, f"every fp16 opacity, {what}")
