"""CPU: the oracle's densify stages against the plain forms of tests/densifycases.py, on exactly the inputs tests/test_gpu_densify_kernels.py
gives the kernels -- and each case doing what it was crafted for.  This is what makes the oracle a fair referee there."""
import numpy as np
import pytest

import densifycases as dc
import indep64 as ind

KEYS = tuple(dc.STATE_WIDTHS)


# ----------------------------------------------------------------------------------------------------------------- K31
@pytest.mark.parametrize("shape", dc.DOWNSAMPLE_SHAPES, ids=dc.downsample_id)
def test_downsample_is_the_linear_sampler(orc, shape):
    """The oracle is floor(v + 0.5) of the float64 filter (v in levels) wherever v + 0.5 is further than 1e-3 from an integer and within one
    level elsewhere; at most 2 % of the texels lie that near (the float32 evaluation error is below 1e-4 of a level: a handful of roundings
    of values below 256).  Measured shares, in the order of DOWNSAMPLE_SHAPES: 0.87 %, 0 %, 0 %, 0 %, 1.14 %, 0 % -- no mismatch outside."""
    (sw, sh), (dw, dh) = shape
    src = dc.downsample_source(shape)
    got = orc.downsample_bilinear(src, dw, dh).astype(np.int64)
    t = dc.downsample_fp64(src, dw, dh) + 0.5
    band = np.abs(t - np.round(t)) <= dc.DOWNSAMPLE_BAND
    share = float(band.mean())
    print(f"down-sample {dc.downsample_id(shape)}: {100 * share:.2f} % of {band.size} texel channels in the band")
    assert share <= dc.DOWNSAMPLE_BAND_SHARE
    diff = np.abs(got - np.floor(t).astype(np.int64))
    assert diff[~band].max(initial=0) == 0 and diff.max() <= 1
    if (sw, sh) == (dw, dh):
        assert np.array_equal(got, src)
    if (sw, sh) == (1, 1):
        assert np.all(got == src[0, 0])
    if dw > sw:     # up-sampling: the outermost texels sample past the edge on all four sides and clamp
        assert np.array_equal(got[0, 0], src[0, 0]) and np.array_equal(got[-1, -1], src[-1, -1])


# ----------------------------------------------------------------------------------------------------------------- K21-K23
@pytest.mark.parametrize("size", dc.METRIC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_metric_map_in_exact_integers(orc, size):
    """The error is an integer channel sum s / 765 scaled by 1e6: the oracle's stored error and its min / max equal the exact floor within
    +-1.  The flags equal the exact comparison (e - min) > t (max - min) at every pixel, because no pixel of any case has an exact norm
    within 1e-5 of a threshold without being ON it, and the ones that are on it -- norm 0 at threshold 0, norm 1 at threshold 1 -- are the
    pixels of smallest and largest error, whose float32 norm is an exact 0 / 1 (the smallest error of every case is an exact 0)."""
    w, h = size
    for kind in dc.METRIC_CONTENTS:
        pred, targ = dc.metric_images(kind, w, h)
        exact = dc.metric_exact(pred, targ)
        assert exact.min() == 0 or kind == "constant" or w * h == 1      # (a single pixel is its own minimum: max == min, nothing flagged)
        for thr in dc.METRIC_THRESHOLDS:
            err, mm, flags = orc.metric_map(pred, targ, thr)
            what = f"{kind} {w}x{h} t={thr}"
            assert np.abs(err.astype(np.int64) - exact).max() <= 1, what
            assert abs(int(mm[0]) - int(exact.min())) <= 1 and abs(int(mm[1]) - int(exact.max())) <= 1, what
            want, dist = dc.metric_flags_exact(exact, thr)
            assert not np.any((dist > 0) & (dist < dc.METRIC_BAND)), f"{what}: a pixel within 1e-5 of the threshold"
            assert np.array_equal(flags, want), what
            if kind in ("identical", "constant", "alpha-only") or w * h == 1:
                assert mm[0] == mm[1] and not flags.any(), what
                assert (mm[0] > 0) == (kind == "constant" or (kind in ("last-pixel", "random") and w * h == 1 and exact.max() > 0)), what
            elif kind == "last-pixel":
                assert flags.sum() == (0 if thr == 1.0 else 1) and (thr == 1.0 or flags[h - 1, w - 1] == 1), what
            else:
                assert (0 < flags.sum() < flags.size) == (thr != 1.0), what


# ----------------------------------------------------------------------------------------------------------------- K24
def _count_flags(orc, kind, W, H):
    if kind != "from-metric-map":
        return dc.count_flags(kind, W, H)
    return orc.metric_map(*dc.count_map_images(W, H), 0.37)[2]


@pytest.mark.parametrize("viewport", dc.COUNT_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_metric_count_between_the_float64_bounds(orc, viewport):
    """Each Gaussian's oracle count lies between the float64 count of walked pairs with alpha >= (1 + 1e-4) / 255 and that with
    alpha >= (1 - 1e-4) / 255; outside the marginal family the two are equal, so the count is exact.  Of the walked pairs (all flags set)
    at least 30 % count and at least 30 % do not, in every viewport of more than one pixel.  Measured, as (walked, counted): 40x24 (35.5 k, 37.5 %),
    17x33 (11.5 k, 31.1 %), 64x64 (134 k, 32.1 %), 1x1 (129, 96 %); no pair outside the marginal family in the band."""
    W, H = viewport
    case = dc.count_case(W, H)
    n, fam, f = case["n"], case["family"], dc.splat_fields(case["splats"], W, H)
    pairs = dc.walked_pairs(case)
    # ---- the case is what it says
    lengths = case["lengths"]
    assert set(lengths) <= {0, 1, 63, 64, 65, 130} and (W * H == 1 or set(lengths) == {0, 1, 63, 64, 65, 130})
    E = case["num_instances"]
    inst = case["instances"][:E]
    assert (inst >= n).any() and case["instances"].size == E + dc.COUNT_TAIL
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert any(np.unique(inst[starts[t]:starts[t + 1]]).size < lengths[t] for t in range(lengths.size))          # a Gaussian twice in a list
    assert np.array_equal(case["ranges"][:-1] == 0xFFFFFFFF, lengths == 0)
    nc, tile_of = case["n_contrib"], case["tile_of"]
    last = tile_of == lengths.size - 1
    assert (nc[last].astype(np.int64) + starts[-2] > E).any(), "no pixel of the last tile walks past num_instances"
    if W * H > 1:
        assert any(np.unique(nc[ys:ys + 8, xs:xs + 8]).size > 8 for ys in range(0, H - 7, 8) for xs in range(0, W - 7, 8)), "n_contrib differs inside a block"
        assert (nc > lengths[tile_of]).any() and (nc[lengths[tile_of] == 0] > 0).any()
    for k in ("cx", "cy", "A", "B", "C", "o"):
        assert not np.isfinite(f[k][fam == "nonfinite"]).all(), k
    needle = fam == "needle"
    assert ((f["A"] * f["C"] - f["B"] ** 2)[needle] <= 0).sum() >= 3, "fp16 rounding left too few needles indefinite"
    outside = (f["cx"] < 0) | (f["cx"] > W) | (f["cy"] < 0) | (f["cy"] > H)
    assert outside.sum() >= 10 and np.nanmax(np.abs(f["cx"][np.isin(fam, ["iso", "aniso"])] - W / 2)) <= W / 2 + 4.1
    if case["attain"]:
        above = 0
        for g, kind, delta, bx, by, ax, ay in case["attain"]:
            ys, xs = np.mgrid[by:by + 8, bx:bx + 8]
            a = dc.alpha255_fp64(f, np.full(64, g), xs.reshape(-1), ys.reshape(-1))
            assert 0.98 <= a.max() <= 1.02 and (a.max() > 1) == (delta > 0) and abs(a.max() - 1) > 2e-3, (g, a.max())
            on_edge = int(ax in (bx, bx + 7)) + int(ay in (by, by + 7))
            assert on_edge == dict(corner=2, edge=1, interior=0)[kind] and a[(ay - by) * 8 + ax - bx] == a.max()
            assert nc[ay, ax] > g, "the attaining pixel does not reach the marginal entry"
            above += delta > 0
        assert above * 2 == len(case["attain"]) == dc.N_MARGINAL
    else:
        assert min(W, H) < 16
    # ---- coverage: all flags set
    counted = ~(pairs[2] < 1.0)
    share = float(counted.mean())
    in_band = np.abs(pairs[2] - 1.0) < 1e-4
    print(f"metric count {W}x{H}: {pairs[0].size} walked pairs, {int(counted.sum())} counted ({100 * share:.1f} %), {int(in_band.sum())} in the band, "
          f"{np.unique(pairs[1][counted]).size} Gaussians with a count")
    assert not in_band[fam[pairs[1]] != "marginal"].any()
    if W * H > 1:
        assert 0.3 <= share <= 0.7
    # ---- the oracle, every flag image, both prefills
    for kind in dc.COUNT_FLAGS:
        flags = _count_flags(orc, kind, W, H)
        low, high = dc.count_bounds(case, pairs, flags)
        assert np.array_equal(low[fam != "marginal"], high[fam != "marginal"])
        for clear in (False, True):
            pre = dc.count_prefill(n, clear)
            counts = np.zeros(n, np.uint32) if clear else pre.copy()
            orc.metric_count(case["settings"], case["ranges"], case["instances"], E, case["splats"], flags, nc, counts)
            got = (counts.astype(np.int64) - (0 if clear else pre.astype(np.int64)))
            assert np.all((low <= got) & (got <= high)), f"{kind}: {np.flatnonzero((got < low) | (got > high))[:5]}"
        if kind == "none":
            assert not high.any()
        if kind == "from-metric-map":
            assert 0 < (flags != 0).sum() < flags.size or W * H == 1


# ----------------------------------------------------------------------------------------------------------------- K25
@pytest.mark.parametrize("n", dc.NORMALIZE_SIZES)
def test_normalize_is_the_integer_quotient(orc, n):
    for d in dc.NORMALIZE_DIVISORS:
        c = dc.normalize_counts(n)
        assert (c == 0).any() or n == 1
        assert (c == 0xFFFFFFFF).any()
        want = dc.normalize_plain(c, d)
        orc.metric_normalize(c, d)
        assert np.array_equal(c, want), (n, d)


# ----------------------------------------------------------------------------------------------------------------- K26
def _decide(orc, g, mc, clone, prune, split):
    p = orc.densify_prepare(g, mc, 0xFFFFFFFF, clone_threshold=clone, prune_opacity=prune, split_scale=split)
    return p["counts"], p["actions"]


def test_decide_over_every_fp16_opacity(orc):
    """All 65 536 patterns at both prune thresholds, with counts on the edges of the clone threshold: no pattern is excused."""
    g, mc = dc.decide_opacity_sweep()
    t = dc.DECIDE_CLONE_THRESHOLD
    for prune in dc.DECIDE_PRUNE_THRESHOLDS:
        for clone, counts in ((t, mc), (0, mc), (t, None)):
            got = _decide(orc, g, counts, clone, prune, 1.0)
            want = dc.decide_plain(g, counts, clone, prune, 1.0)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (prune, clone)
            a = want[1]
            assert (a == 3).sum() > 10000 and (a != 3).sum() > 10000
            assert set(np.unique(a)) == ({3, 1} if clone == 0 else {3, 0} if counts is None else {3, 0, 1})
        a = dc.decide_plain(g, mc, t, prune, 1.0)[1]
        kept = a != 3
        assert np.array_equal(a[kept] == 1, (mc[kept] >= t)) and {int(x) for x in mc} == {t - 1, t, t + 1, 0, 0xFFFFFFFF}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_decide_over_every_fp16_scale(orc, axis):
    g, mc = dc.decide_scale_sweep(axis)
    for split in dc.DECIDE_SPLIT_THRESHOLDS:
        got = _decide(orc, g, mc, dc.DECIDE_CLONE_THRESHOLD, 0.15, split)
        want = dc.decide_plain(g, mc, dc.DECIDE_CLONE_THRESHOLD, 0.15, split)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), split
        assert np.all(want[0] == 2) and (want[1] == 2).sum() > 10000 and (want[1] == 1).sum() > 10000
    nan = np.isnan(ind.unpack_gaussians(g)["log_scale"][:, axis])
    assert nan.sum() == 2046 and np.all(want[1][nan] == 1)       # a NaN scale never splits


# ----------------------------------------------------------------------------------------------------------------- K27-K28
@pytest.mark.parametrize("n", dc.CAP_SIZES)
def test_cap_scans_and_total_are_the_integer_rule(orc, n):
    g, mc, kind = dc.cap_cloud(n)
    dcounts, dactions = dc.decide_plain(g, mc, 6, 0.15, 0.05)
    assert np.array_equal(dcounts, np.array([0, 1, 2, 2])[kind]) and np.array_equal(dactions, np.array([3, 0, 1, 2])[kind])
    assert n == 1 or set(np.unique(dcounts)) == {0, 1, 2}
    values = dc.cap_values(dcounts)
    assert set(values) == ({"0", "1", "2", "total", "total+1", "max", "pair-first-slot"} | ({"single"} if n > 1 else set()))
    total = int(dcounts.sum())
    for name, max_out in values.items():
        p = orc.densify_prepare(g, mc, max_out, clone_threshold=6, prune_opacity=0.15, split_scale=0.05)
        c, a, o, t = dc.cap_plain(dcounts, dactions, max_out)
        assert np.array_equal(p["counts"], c) and np.array_equal(p["actions"], a) and np.array_equal(p["offsets"], o) and p["total"] == t, (n, name)
        assert t == min(total, max_out) or name == "pair-first-slot"
        if name == "pair-first-slot":
            cut = np.flatnonzero((dcounts == 2) & (c == 1))
            assert cut.size == 1 and a[cut[0]] == 0 and t == max_out and not c[cut[0] + 1:].any()
        if name == "single":
            assert t == max_out and np.array_equal(c[c != 0], dcounts[:np.flatnonzero(c)[-1] + 1][dcounts[:np.flatnonzero(c)[-1] + 1] != 0])
        if name in ("total", "total+1", "max"):
            assert np.array_equal(c, dcounts) and np.array_equal(a, dactions)
        if name == "0":
            assert not c.any() and np.all(a == 3)


def test_max_out_points_rule():
    assert dc.max_out_plain(0, 0, 0) == 2 and dc.max_out_plain(4097, 9600, 0) == 100 and dc.max_out_plain(257, 0, 40) == 297
    assert dc.max_out_plain(257, 0, 1) == 258 and dc.max_out_plain(64, 9600, 40) == 100 and dc.max_out_plain(1, 9600, 1) == 2


# ----------------------------------------------------------------------------------------------------------------- K29 + K30
def _ulp_or_abs(got16, want, scale):
    """fp16 result against a float64 value: within one ulp, or (a coordinate near zero is the difference of O(scale) float32 numbers)
    within 2e-6 scale; a NaN where and only where the float64 form has one."""
    got = got16.view(np.float16).astype(np.float64)
    nan = np.isnan(want)
    ok = (ind.f16_ulp_distance(got16, ind.f16_bits(np.where(nan, 0, want))) <= 1) | (np.abs(got - want) <= 2e-6 * scale)
    return bool(np.array_equal(np.isnan(got), nan) and ok[~nan].all())


def check_scatter(orc, g, sh, st, tables, reset):
    """The oracle's scatter against the plan (integers: which slot takes which row, reset or carry, exact copies) and the float64
    children; unwritten slots stay zero."""
    counts, actions, offsets, out_n = tables
    og, osh, ost = orc.densify_scatter(g, sh, st, dict(offsets=offsets, counts=counts, actions=actions), out_n, reset)
    dst, src, variant = dc.scatter_plan(counts, offsets, out_n)
    a = actions[src]
    hole = np.ones(out_n, bool)
    hole[dst] = False
    assert not og[hole].any() and not osh[hole].any() and not any(ost[k][hole].any() for k in KEYS)
    assert np.array_equal(osh[dst], sh[src])
    gin, gout, gs = dc.halves(g)[src], dc.halves(og)[dst], ind.unpack_gaussians(g)
    moved = (a == 2) | ((a == 1) & (variant == 1))
    with np.errstate(over="ignore", invalid="ignore"):
        clamped = ind.sigmoid(gs["opacity_raw"][src]) > dc.OPACITY_MAX
    repacked = moved | clamped
    is_nan16 = lambda b: ((b & 0x7C00) == 0x7C00) & ((b & 0x3FF) != 0)
    same = lambda x, y: np.array_equal(is_nan16(x), is_nan16(y)) and np.array_equal(x[~is_nan16(y)], y[~is_nan16(y)])
    assert np.array_equal(gout[:, 4:8], gin[:, 4:8])
    assert np.array_equal(gout[:, 11], np.where(a == 2, 0, gin[:, 11]))
    assert same(gout[:, 3], np.where(clamped, ind.f16_bits(dc.OPACITY_MAX_RAW), gin[:, 3]))
    assert np.array_equal(gout[~repacked][:, [0, 1, 2, 3, 8, 9, 10]], gin[~repacked][:, [0, 1, 2, 3, 8, 9, 10]])
    assert same(gout[~moved][:, 0:3], gin[~moved][:, 0:3]) and np.array_equal(gout[a != 2][:, 8:11], gin[a != 2][:, 8:11])
    pos, quat, ls = gs["pos"][src], gs["quat"][src], gs["log_scale"][src]
    with np.errstate(all="ignore"):
        want_pos, want_ls = dc._densify_children_fp64(pos, quat, ls, src, dst, a, variant)
        nan_in = np.isnan(quat).any(1) | np.isnan(ls).any(1)
        null_q = (quat * quat).sum(1) < 1e-12          # normalised with the 1e-12 floor it stays (near) zero: the offset vanishes
        want_pos[moved & nan_in] = np.nan
        want_pos[moved & null_q & ~nan_in] = pos[moved & null_q & ~nan_in]
        scale = np.maximum(1.0, np.abs(pos).max(1) + 2.0 * np.exp(np.clip(np.nan_to_num(ls), -10, 10)).max(1))[:, None]
    assert _ulp_or_abs(gout[moved][:, 0:3], want_pos[moved], scale[moved])
    assert _ulp_or_abs(gout[a == 2][:, 8:11], want_ls[a == 2], 0.0)
    if moved.any() and np.isfinite(want_pos[moved]).all():
        assert (np.abs(gout[moved][:, 0:3].view(np.float16).astype(np.float64) - pos[moved]).max(1) > 0).mean() > 0.9
    # ---- fp32 masters
    new = (variant == 1) | (a == 2)
    rst = (new & bool(reset))[:, None]
    u = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for k in ("opt_pos", "opt_rot", "opt_scale"):
        assert np.array_equal(u(ost[k][dst, 4:]), np.where(rst, 0, u(st[k][src, 4:]))), k
    assert np.array_equal(u(ost["state_sh"][dst]), np.where(rst, 0, u(st["state_sh"][src])))
    assert np.array_equal(u(ost["param_sh"][dst]), u(st["param_sh"][src])) and np.array_equal(u(ost["opt_rot"][dst, 0:4]), u(st["opt_rot"][src, 0:4]))
    assert np.array_equal(u(ost["opt_pos"][dst, 3]), u(st["opt_pos"][src, 3])) and np.array_equal(u(ost["opt_scale"][dst, 3]), u(st["opt_scale"][src, 3]))
    assert not u(ost["opt_opacity"][dst, 1:]).any()
    raw = st["opt_opacity"][src, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        clamp64 = ind.sigmoid(raw.astype(np.float64)) > dc.OPACITY_MAX
    want_raw = np.where(clamp64, dc.OPACITY_MAX_RAW, raw)
    got_raw = ost["opt_opacity"][dst, 0]
    ladder = np.abs(raw.astype(np.float64) - float(dc.OPACITY_MAX_RAW)) < 2e-6          # float32 rounding of the sigmoid decides there
    assert np.array_equal(u(got_raw[~ladder]), u(want_raw[~ladder]))
    assert np.all((u(got_raw[ladder]) == u(raw[ladder])) | (got_raw[ladder] == dc.OPACITY_MAX_RAW))
    assert np.array_equal(u(ost["opt_pos"][dst][~moved][:, 0:3]), u(st["opt_pos"][src][~moved][:, 0:3]))
    assert np.array_equal(u(ost["opt_scale"][dst][a != 2][:, 0:3]), u(st["opt_scale"][src][a != 2][:, 0:3]))
    mp, mq, ms = (st[k][src, 0:w].astype(np.float64) for k, w in (("opt_pos", 3), ("opt_rot", 4), ("opt_scale", 3)))
    with np.errstate(all="ignore"):
        m_pos, _ = dc._densify_children_fp64(mp, mq, ms, src, dst, a, variant)
        nan_in = np.isnan(mq).any(1) | np.isnan(ms).any(1)
        null_q = (mq * mq).sum(1) < 1e-12
        m_pos[moved & nan_in] = np.nan
        m_pos[moved & null_q & ~nan_in] = mp[moved & null_q & ~nan_in]
        scale = np.maximum(1.0, np.abs(mp).max(1) + 2.0 * np.exp(np.clip(np.nan_to_num(ms), -10, 10)).max(1))[:, None]
        got_pos = ost["opt_pos"][dst, 0:3].astype(np.float64)
        assert np.array_equal(np.isnan(got_pos[moved]), np.isnan(m_pos[moved]))
        assert np.all((np.abs(got_pos - m_pos) <= 4e-6 * scale)[moved & ~np.isnan(m_pos).any(1)])
        got_s, want_s = ost["opt_scale"][dst, 0:3].astype(np.float64)[a == 2], ms[a == 2] - dc.LN_1P6
        fin = np.isfinite(want_s)
        assert np.array_equal(got_s[~fin], want_s[~fin], equal_nan=True) and np.all(np.abs(got_s - want_s)[fin] <= 1e-6 * np.maximum(1.0, np.abs(want_s[fin])))
    return dst, src, variant, a


@pytest.mark.parametrize("name,n", dc.SCATTER_CASES, ids=[f"{k}-{n}" for k, n in dc.SCATTER_CASES])
def test_scatter_tables(orc, name, n):
    g, sh, st = dc.scatter_cloud(n)
    tables = dc.scatter_tables(name, n)
    counts, actions, offsets, out_n = tables
    for reset in (True, False):
        dst, src, variant, a = check_scatter(orc, g, sh, st, tables, reset)
    total = int(np.where(counts == 0, 0, np.where(counts == 2, 2, 1)).sum())
    if name == "mixed":
        assert dst.size == out_n == total or total == 0
        assert n < 63 or {0, 1, 2, 3} <= set(actions)
    if name == "waves":
        live = (counts != 0).reshape(-1, 1)[:320].reshape(5, 64)
        assert not live[0].any() and live[1].all() and np.all(actions[64:128] == 2)
        assert np.flatnonzero(live[2]).tolist() == [0] and np.flatnonzero(live[3]).tolist() == [63] and n % 64 != 0
    if name == "short":
        straddle = np.flatnonzero((counts == 2) & (offsets == out_n - 1))
        assert straddle.size == 1 and dst.size == out_n < total and src[-1] == straddle[0] and variant[-1] == 0
        assert (counts[straddle[0] + 1:] != 0).any()
    if name == "long":
        assert dst.size == total == out_n - 7
    if name == "odd":
        assert dst.size < out_n and (n <= 8 or (offsets[counts != 0] >= out_n).any())
        if n > 8:
            assert {3, 0xFFFFFFFF} <= set(counts[src].tolist()) and ((actions[src] == 0) & (variant == 1)).any()
            assert ((actions[src] == 3) & (counts[src] == 1)).any() and (actions[src] == 7).any()
    if n == 5000:
        assert (src * 1664525 >= 1 << 32).any() and (src * 747796405 >= 1 << 32).any()


@pytest.mark.parametrize("what", ["keep", "clone", "split"])
def test_scatter_value_edges(orc, what):
    g, sh, st = dc.value_cloud()
    n = g.shape[0]
    for reset in (True, False):
        check_scatter(orc, g, sh, st, dc.value_tables(n, what), reset)
    gs = ind.unpack_gaussians(g)
    assert np.isinf(gs["pos"]).sum() == 0 and (np.abs(gs["pos"]) > 5e4).any() and np.isnan(gs["quat"]).any() and np.isnan(gs["log_scale"]).any()
    assert np.isinf(gs["log_scale"]).any() and (gs["log_scale"] > 10).any() and (gs["log_scale"] < -10).any() and ((gs["quat"] ** 2).sum(1) == 0).any()
    raw = st["opt_opacity"][:, 0]
    assert (np.abs(raw.astype(np.float64) - float(dc.OPACITY_MAX_RAW)) < 2e-6).sum() == 17 and np.isnan(raw).any() and np.isinf(raw).sum() == 2


@pytest.mark.parametrize("what", ["keep", "split"])
def test_scatter_over_every_fp16_opacity(orc, what):
    """The clamp of the working copy over all 65 536 raw opacities, on the untouched path (keep) and the re-packed one (split): the oracle
    agrees with float64 on every pattern (check_scatter excuses none)."""
    g, sh, st = dc.opacity_sweep_cloud()
    check_scatter(orc, g, sh, st, dc.value_tables(g.shape[0], what), True)
