"""CPU: the crafted raster cases (tests/rastercases.py) -- the parity oracle's rasterize and backward_rasterize held to the float64 restatement on
every case, and every case held to what it claims to reach.  The GPU side (tests/test_gpu_raster_kernels.py) compares the kernels with the oracle
bit for bit on the same cases; this file is what makes the oracle worth comparing with at these corners.

Forward, outside the excused pixels: n_contrib exact, rgba8 within one level, final T within 1e-5 (the bounds of test_oracle_golden.py's float64
re-composite).  A pixel is excused when one of its decisions lies within 1e-4 (relative) of its threshold -- alpha against 1/255, the running A
against the 0.99 stop: float64 cannot call those.  Their share of the covered pixels is at most 10 % per case outside family 3, which is made of them.

Backward: the loss gradient of the excused pixels is zeroed in the image pair handed to BOTH sides, then the oracle's i32 sums are compared with the
float64 sums -- modulo 2^32, as i32 sums wrap -- both fed the oracle's own final T and n_contrib.  The allowance per Gaussian and slot is one unit per
contributing (pixel, splat) pair (each contribution is truncated) plus REL_BOUND times the largest sum of absolute contributions of that array in the case.  REL_MEASURED is the
oracle's largest such distance over all cases, measured here; the bound is four times it and must stay below 1e-3, so that a wrong sign, a missing
factor 2 or a dropped term cannot hide under it.  Cases with a contribution that saturates the fixed-point conversion -- or, by design, wraps -- are
excluded from the float64 comparison by name (f64_backward = False: family 7's three, and the indefinite conics of family 5, whose exp(87) overflows
float32 products); the oracle still runs on them here, and the GPU test compares their bits."""
import ctypes

import numpy as np
import pytest

import rastercases as rc

REL_MEASURED = 1.5e-5   # the 2049-tile row, conic sums: at 32 784 px a float32 pixel-space centre is 1e-3 px off; every other case stays inside the truncation allowance
REL_BOUND = 4.0 * REL_MEASURED

CASES = rc.all_cases()
IDS = [c["name"] for c in CASES]
_cache = {}


def oracle_forward(orc, case):
    """(rgba8, final T, n_contrib, float64 forward) of a case, computed once."""
    if case["name"] not in _cache:
        rows = np.ascontiguousarray(case["rows"][:case["num_splats"]])
        out = orc.rasterize(rc.settings_array(case), rc.tile_info_array(case), rows, case["ranges"], case["keys"], case["vals"], case["count"], case["max_batches"])
        _cache[case["name"]] = out + (rc.forward64(case),)
    return _cache[case["name"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_against_float64(orc, case):
    rgba, T, ncon, f = oracle_forward(orc, case)
    keep = ~f["excused"]
    covered = int(f["covered"].sum())
    if case["family"] != 3 and covered:
        assert (f["excused"] & f["covered"]).sum() <= 0.10 * covered, "too many pixels excused for the check to mean much"
    assert np.array_equal(ncon[keep], f["n_contrib"][keep]), "n_contrib"
    want = np.floor(np.clip(f["C"], 0.0, 1.0) * 255.0 + 0.5)
    assert np.abs(rgba[:, :, :3].astype(np.float64) - want)[keep].max(initial=0) <= 1, "rgba8"
    assert (rgba[:, :, 3] == 255).all()
    assert np.abs(T.astype(np.float64) - f["T"])[keep].max(initial=0) < 1e-5, "final T"


def backward_pair(orc, case):
    """(the oracle's four i32 arrays, the float64 four, pairs per Gaussian, abs sums[N, 9]) with the excused pixels' gradient zeroed on both sides."""
    _, T, ncon, f = oracle_forward(orc, case)
    targ = case["targ"].copy()
    targ[f["excused"]] = case["pred"][f["excused"]]
    lg = orc.loss_grad(case["pred"], targ, orc.training_config(0.0, case["lam"], 0.0))
    assert not lg[f["excused"]][:, :3].any()
    got = orc.backward_rasterize(rc.settings_array(case, backward=True), case["rows"].shape[0], case["ranges"], case["vals"], case["rows"], T, ncon, lg)
    with np.errstate(all="ignore"):
        sums, pairs, asums = rc.backward64(case, T, ncon, rc.loss_gradient64(case, targ=targ))
    return got, rc.reference_layout(sums), pairs, asums


def distances(got, want, pairs, asums):
    """Per array: the largest excess of |oracle - float64| over the truncation allowance, relative to the array's largest sum of absolute contributions."""
    per = (np.repeat(pairs, 2), np.repeat(pairs, 4), pairs, np.repeat(pairs, 3))
    scale = (asums[:, 0:2].max(), asums[:, 2:5].max(), asums[:, 5].max(), asums[:, 6:9].max())
    out = []
    for g, w, p, s in zip(got, want, per, scale):
        diff = (g.astype(np.float64) - w + 2.0 ** 31) % 2.0 ** 32 - 2.0 ** 31     # i32 sums wrap, as atomicAdd's do: compared modulo 2^32
        excess = np.maximum(np.abs(diff) - p, 0.0).max(initial=0)
        out.append(excess / s if s > 0 else (0.0 if excess == 0 else np.inf))
    return out


BACKWARD = [c for c in CASES if c["k16"] and c["mode"] == 1]


@pytest.mark.parametrize("case", BACKWARD, ids=[c["name"] for c in BACKWARD])
def test_backward_against_float64(orc, case):
    got, want, pairs, asums = backward_pair(orc, case)
    unlisted = np.setdiff1d(np.arange(case["rows"].shape[0]), case["vals"])
    for a, width in zip(got, (2, 4, 1, 3)):
        assert not a.reshape(-1, width)[unlisted].any(), "a Gaussian in no list has a sum"
    if not case["f64_backward"]:
        return   # saturated or wrapped sums: the oracle ran, the GPU test compares bits
    d = distances(got, want, pairs, asums)
    print(f"{case['name']}: relative distance per array {d}")
    # the whole allowance stays below 1e-3 of the case's largest sum (and, the comparison being modulo 2^32, far below 2^31)
    scale = max(asums[:, 0:2].max(), asums[:, 2:5].max(), asums[:, 5].max(), asums[:, 6:9].max())
    if scale == 0.0:   # (a list that covers no pixel)
        assert not any(a.any() for a in got)
        return
    assert REL_BOUND < 1e-3 and pairs.max() + REL_BOUND * scale < min(1e-3 * scale, 2.0 ** 28), (pairs.max(), scale)
    assert max(d) <= REL_BOUND, d


def test_measured_distance_is_the_one_written_down(orc):
    """REL_MEASURED is the largest distance over all cases (so the bound is four times what the oracle does, not a guess)."""
    worst = max(max(distances(*backward_pair(orc, c))) for c in BACKWARD if c["f64_backward"])
    print("largest relative distance:", worst)
    assert 0.5 * REL_MEASURED <= worst <= REL_MEASURED


# ----------------------------------------------------------------------------- each case reaches what it names
def test_family_1_reaches_its_compacted_counts():
    seen = set()
    for c in rc.family(1):
        counts = rc.compacted_counts(c)
        for v in counts.values():
            seen.update(v)
        for at, want in c["claims"].get("counts", {}).items():
            assert counts[at] == want, (c["name"], at, counts[at])
    assert {0, 1, 2, 64} <= seen and any(v % 2 and v > 2 for v in seen) and any(v % 2 == 0 and 2 < v < 64 for v in seen)
    table = rc.compacted_counts(next(c for c in rc.family(1) if c["name"] == "chunk table"))
    assert any(v[1:-1].count(0) and v[0] and v[-1] for v in table.values()), "a middle chunk that keeps nothing"
    assert any(not any(v[:-1]) and v[-1] for v in table.values()), "a block whose only kept records are in the last chunk"
    exactly_one = 0
    for c in rc.family(1):
        u, ntx = rc._geometry(c), (c["W"] + 15) // 16
        for t in np.flatnonzero(c["ranges"][:-1] != rc.EMPTY):
            for g in rc.forward_list(c, t):
                hit = 0
                for sub in range(4):
                    bx, by = 16 * (t % ntx) + 8 * (sub & 1), 16 * (t // ntx) + 8 * (sub >> 1)
                    hit += not (bx + 0.5 - u["cx"][g] > u["ex"][g] or u["cx"][g] - bx - 7.5 > u["ex"][g] or by + 0.5 - u["cy"][g] > u["ey"][g] or u["cy"][g] - by - 7.5 > u["ey"][g])
                exactly_one += hit == 1
    assert exactly_one > 100
    lens = {}
    for c in rc.family(1):
        r = c["ranges"]
        T = r.size - 1
        for t in range(T):
            if r[t] != rc.EMPTY:
                nxt = next((int(r[u]) for u in range(t + 1, T + 1) if r[u] != rc.EMPTY), c["count"])
                lens.setdefault(c["name"], []).append((t, nxt - int(r[t]), T))
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 193} - {0} <= {n for v in lens.values() for _, n, _ in v}
    full = lens["full chunks then the next tile"]
    assert any(n == 64 and t + 1 < T for t, n, T in full) and any(n == 128 for _, n, _ in full)
    assert any(n % 64 for _, n, _ in lens["key change mid-chunk"])
    assert lens["only the last tile"][0][0] == lens["only the last tile"][0][2] - 1 and lens["only the first tile"][0][0] == 0


def test_family_1_sentinels_are_where_they_claim(orc):
    c = next(c for c in rc.family(1) if c["name"] == "values beyond num_splats")
    start1 = int(c["ranges"][1])
    l0 = c["vals"][:start1]
    ghosts = np.flatnonzero(l0 >= c["num_splats"])
    assert ghosts[0] == 0 and 0 < ghosts[1] < 63 and ghosts[2] == 64 and ghosts.size == 4
    # they are counted by neither side: the n_contrib of a pixel every real record of tile 0 reaches is below the list length by the ghosts in front
    _, _, ncon, f = oracle_forward(orc, c)
    assert ncon[:, :16].max() <= l0.size - ghosts.size and np.array_equal(ncon, f["n_contrib"])
    c = next(c for c in rc.family(1) if c["name"].startswith("a batch of values"))
    assert rc.forward_list(c, 0).size == c["claims"]["forward_entries"] and oracle_forward(orc, c)[2].max() == 3


def test_family_2_saturates_where_it_says(orc):
    for c in rc.family(2):
        _, T, ncon, f = oracle_forward(orc, c)
        cl = c["claims"]
        if "saturated_at" in cl:
            for b in cl["blocks"]:
                blk = ncon[8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8]
                assert (blk == cl["saturated_at"]).all() and (f["A"][8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8] > rc.STOP).all(), c["name"]
            others = [b for b in range(4) if b not in cl["blocks"]]
            for b in others:
                assert ncon[8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8].min() > cl["saturated_at"], c["name"]
        if "smallest_T_at" in cl:
            y, x = cl["smallest_T_at"]
            assert T[y, x] == T.min() and 0.9e-4 < T[y, x] < 1.1e-4 and ncon[y, x] == 2
        if "distinct_n_contrib" in cl:
            assert min(np.unique(ncon[8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8]).size for b in range(4)) >= cl["distinct_n_contrib"]


def _pairs(case):
    """For every (pixel, composited entry) of a case: the exponent's argument and opacity * G, float64."""
    u = rc._geometry(case)
    args, ogs = [], []
    for t in np.flatnonzero(case["ranges"][:-1] != rc.EMPTY):
        g = rc.forward_list(case, t)
        ys, xs = rc._tile_pixels(case, t)
        dx, dy, inside, G, _ = rc._alpha(u, g, xs + 0.5, ys + 0.5)
        c = u["conic"][g]
        arg = -0.5 * (c[None, :, 0] * dx * dx + 2.0 * c[None, :, 1] * dx * dy + c[None, :, 2] * dy * dy)
        args.append(arg[inside])
        ogs.append((u["op"][g][None, :] * G)[inside])
    return np.concatenate(args), np.concatenate(ogs)


def test_family_3_straddles_its_thresholds(orc):
    by = {c["name"]: c for c in rc.family(3)}
    _, og = _pairs(by["alpha across 1/255"])
    assert (og < rc.MIN_ALPHA).sum() > 50 and (og >= rc.MIN_ALPHA).sum() > 50 and (np.abs(og / rc.MIN_ALPHA - 1) < 0.2).sum() > 10
    _, og = _pairs(by["alpha across 0.99"])
    assert (og < rc.STOP).sum() > 50 and (og > rc.STOP).sum() > 20
    _, og = _pairs(by["centred on a pixel, lowest opacity"])
    assert np.isclose(og.max(), 1.0) and np.any(og == float(rc.f16_step(1.0 / 128.0, 1)))
    # the three alphas that EQUAL 1/255 in float32, with the oracle's exp
    for a, c, dx, dy, op in rc.EXACT_MIN_ALPHA:
        assert all(float(rc.f16v(v)) == v for v in (a, c, op))
        xe = np.array([(-0.5 * a * dx) * dx + (-0.5 * c * dy) * dy], np.float32)   # (both products exact in float32, their sum rounded once: the kernels' FMA chain)
        G = np.zeros(1, np.float32)
        orc.lib().orc_test_exp(ctypes.c_uint32(1), xe.ctypes.data_as(ctypes.c_void_p), G.ctypes.data_as(ctypes.c_void_p))
        assert np.float32(G[0] * np.float32(op)) == np.float32(1.0 / 255.0)
    case = by["alpha equal to 1/255"]
    y, x = case["claims"]["exact_min_alpha"]
    assert oracle_forward(orc, case)[2][y, x] == len(rc.EXACT_MIN_ALPHA)   # the last of them still counts: >= 1/255


def test_family_4_rings_and_caps(orc):
    by = {c["name"]: c for c in rc.family(4)}
    _, _, ncon, _ = oracle_forward(orc, by["extent equal to |d|, a half either side, zero"])
    for i, reach in enumerate((2, 1, 2, 0)):   # |d| == extent is inside; one half below it is not; extent 0 keeps the centre pixel alone
        oy, ox = 16 * (i // 2), 16 * (i % 2)
        hit = ncon[oy:oy + 16, ox:ox + 16] > 0
        want = np.zeros((16, 16), bool)
        want[8 - reach:9 + reach, 8 - reach:9 + reach] = True
        for y in (3, 4):                             # the second splat: two pixel rows at |dy| = 0.5 exactly, its x extent as the first one's
            want[y, 4 - reach:5 + reach] = True
        assert np.array_equal(hit, want), i
    capped = oracle_forward(orc, by["extent above the cap, default cap"])[2]
    lifted = oracle_forward(orc, by["extent above the cap, cap lifted"])[2]
    assert capped[8, 128] > 0 and capped[8, 129] == 0 and lifted[8, 129] > 0 and lifted[8, 200] > 0
    assert (oracle_forward(orc, by["centres outside the image"])[2] > 0).sum() > 40


def test_family_5_reaches_its_arguments():
    for c in rc.family(5):
        args, _ = _pairs(c)
        for lo, hi in c["claims"].get("arguments", ()):
            assert np.any(args == lo) if lo == hi else np.any((args > lo) & (args < hi)), (c["name"], lo, hi)
    args, _ = _pairs(rc.family(5)[0])
    assert args.min() < -100 and np.any((args < 0) & (args > -1e-4))


def test_family_6_sits_on_the_contour_and_the_cull_sees_both_sides():
    case = rc.family(6)[0]
    u = rc._geometry(case)
    kinds = {"none": 0, "corner": 0, "edge": 0, "more": 0}
    verdict = {"dropped": 0, "kept inside the margin": 0, "kept above the threshold": 0}
    sides = set()
    for e in case["claims"]["cull"]:
        g, bx, by = e["g"], e["bx"], e["by"]
        ys, xs = np.mgrid[by:by + 8, bx:bx + 8]
        _, _, _, G, _ = rc._alpha(u, np.array([g]), (xs + 0.5).reshape(-1), (ys + 0.5).reshape(-1))
        a = (u["op"][g] * G[:, 0]).reshape(8, 8)
        assert abs(a.max() * 255.0 - 1.0) <= 0.021, e
        over = a >= rc.MIN_ALPHA
        if over.sum() == 0:
            kinds["none"] += 1
        elif over.sum() > 1:
            kinds["more"] += 1
        else:
            y, x = np.argwhere(over)[0]
            kinds["corner" if (y in (0, 7) and x in (0, 7)) else "edge" if (y in (0, 7) or x in (0, 7)) else "more"] += 1
        cx, cy = u["cx"][g], u["cy"][g]
        sides.add((int(cx > bx + 7.5) - int(cx < bx + 0.5), int(cy > by + 7.5) - int(cy < by + 0.5)))
        A, B, C = u["conic"][g]
        qmin, thr, margin = rc.block_cull(A, B, C, u["op"][g], bx + 0.5 - cx, bx + 7.5 - cx, by + 0.5 - cy, by + 7.5 - cy)
        verdict["dropped" if qmin > thr + margin else "kept inside the margin" if qmin > thr else "kept above the threshold"] += 1
        if qmin > thr + margin:
            assert over.sum() == 0, "the restated cull drops a record with a contributing pixel"
    assert len(case["claims"]["cull"]) >= 300 and min(kinds[k] for k in ("none", "corner", "edge")) >= 10, kinds
    assert min(verdict.values()) >= 5, verdict
    assert len(sides) == 8, sides


def test_family_7_wraps_and_saturates(orc):
    for c in rc.family(7):
        if not c["claims"].get("wraps") and not c["claims"].get("wraps_across"):
            continue
        _, T, ncon, _ = oracle_forward(orc, c)
        with np.errstate(all="ignore"):
            sums, pairs, asums = rc.backward64(c, T, ncon, rc.loss_gradient64(c))
        assert np.abs(sums).max() > 2.0 ** 31, c["name"]
        per_pixel = asums.max() / max(pairs.max(), 1)
        if "saturates" in c["name"]:
            assert per_pixel > 2.0 ** 31
        if c["claims"].get("wraps_across"):   # no wave of 64 pixels wraps on its own in the colour slots: the sum over the tiles does
            assert asums[:, 6:9].max() / (pairs.max() / 64.0) < 2.0 ** 31 < asums[:, 6:9].max()
    c = next(c for c in rc.family(7) if "unlisted" in c["name"])
    assert np.setdiff1d(np.arange(40), c["vals"]).tolist() == c["claims"]["unlisted"] and np.any(np.diff(c["vals"].astype(np.int64)) < 0)


def test_family_8_grids():
    tiles = sorted({(c["W"] + 15) // 16 * ((c["H"] + 15) // 16) for c in rc.family(8)})
    assert {1, 7, 8, 9, 17, 2049} <= set(tiles)
    assert sorted(c["count"] for c in rc.family(8) if c["max_batches"] == 1) == [255, 256, 257, 300]
    assert sum(c["mode"] == 0 for c in rc.family(8)) == 2
