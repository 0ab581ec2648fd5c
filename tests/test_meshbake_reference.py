"""CPU: the restatement of vertex-colour baking (tests/meshbake_ref.py) against properties that need no floats: a constant photograph gives exactly its
colour, a vertex on a texel centre exactly that texel, the ramp image exactly the position, any order of the views the same state, no texel outside the
image is read, and the crafted cases hit what they are crafted for."""
import itertools

import numpy as np
import pytest

import meshbake_ref as B
import meshraster_ref as R

F32 = np.float32


def _constant(W, H, rgba):
    return np.broadcast_to(np.array(rgba, np.uint8), (H, W, 4)).copy()


@pytest.mark.parametrize("name", ["random-256-67x45", "random-257-67x45-depth-normals", "random-1000-67x45-depth", "random-1000-5x3-normals", "weight-rule", "borders-2x2"])
def test_a_constant_photograph_gives_exactly_its_colour(name):
    m = B.case(name)
    rgba = (201, 3, 77, 9)
    views = [dict(w, image=_constant(w["width"], w["height"], rgba)) for w in m["views"]]
    out = B.run(dict(m, views=views))
    assert out["baked"].any(), "the case bakes something"
    assert np.all(out["colours"][out["baked"]] == np.array([201, 3, 77, 255], np.uint8)), "a baked vertex has the photograph's colour and alpha 255"
    if m["fallback"] is not None:
        assert np.array_equal(out["colours"][~out["baked"]], m["fallback"][~out["baked"]]), "any other vertex keeps its fallback"
    sums = out["sums"].astype(object)
    for ch, byte in enumerate(rgba[:3]):   # every view adds Q (256 byte): the sums themselves are exact
        assert all(int(r[ch]) == 256 * byte * int(r[3]) for r in sums)


def test_a_vertex_on_a_texel_centre_gets_exactly_that_texel():
    W, H = 8, 4   # (powers of two: `pixel` places exactly)
    image = B.noise_image(W, H, 1)
    centres = [(i, j) for j in range(H) for i in range(W)]
    v = [B.pixel(256 * i, 256 * j, 1.0 + 0.125 * ((i + j) % 3), W, H) for i, j in centres]
    state = B.accumulate(B.new_state(len(v)), v, None, R.crafted_camera(W, H), image, None, W, H)
    assert state["totals"]["accumulated"] == len(v)
    colours, baked = B.resolve(state)
    assert baked.all()
    for k, (i, j) in enumerate(centres):
        assert state["sums"][k] == [256 * 256 * int(image[j, i, ch]) for ch in range(3)] + [256]
        assert colours[k].tolist() == image[j, i, :3].tolist() + [255]


def test_the_ramp_image_gives_the_position_exactly():
    W, H = 64, 32
    image = B.ramp_image(W, H)
    rng = np.random.default_rng(3)
    for _ in range(200):
        xs, ys = int(rng.integers(0, 256 * (W - 1) + 1)), int(rng.integers(0, 256 * (H - 1) + 1))
        texels, weights = B.footprint(xs, ys, W, H)
        assert sum(weights) == 65536
        S, s = B.sample(image, texels, weights)
        assert S[0] == 256 * (3 * xs + 2 * ys), "S = 256 (3 X' + 2 Y') on T(i, j) = 3 i + 2 j"
        assert S[1] == 65536 * 255 - S[0] and S[2] == 256 * ys
        assert s[0] == (S[0] + 128) >> 8 == 3 * xs + 2 * ys
    # and through accumulate: a vertex `pixel` puts at (X', Y')
    v = [B.pixel(1000, 517, 2.0, W, H), B.pixel(256 * (W - 1), 256 * (H - 1), 1.0, W, H), B.pixel(0, 0, 3.0, W, H)]
    state = B.accumulate(B.new_state(3), v, None, R.crafted_camera(W, H), image, None, W, H)
    assert [r[0] for r in state["sums"]] == [256 * (3 * 1000 + 2 * 517), 256 * (3 * 256 * (W - 1) + 2 * 256 * (H - 1)), 0]


def test_any_order_of_three_views_gives_the_same_state():
    m = B.case(B.THREE_VIEWS)
    assert len(m["views"]) == 3
    first = B.run(m)
    assert first["totals"]["accumulated"] > 100 and first["views"].max() >= 2
    for order in itertools.permutations(range(3)):
        out = B.run(m, order)
        for k in ("sums", "views", "colours", "baked"):
            assert np.array_equal(out[k], first[k]), (order, k)
        assert out["totals"] == first["totals"]


def test_the_far_edge_clamps_and_no_texel_outside_the_image_is_read():
    for W, H in B.SIZES + ((8, 4),):
        xm, ym = 256 * (W - 1), 256 * (H - 1)
        texels, weights = B.footprint(xm, ym, W, H)
        assert texels == [(W - 1, H - 1)] * 4 and weights == [65536, 0, 0, 0], "at X' = 256 (W - 1) i1 clamps onto i0 and a = 0"
        for xs, ys in ((0, 0), (xm, 0), (0, ym), (min(xm // 2 + 1, xm), min(ym // 2 + 1, ym)), (max(xm - 1, 0), max(ym - 1, 0))):
            texels, weights = B.footprint(xs, ys, W, H)
            assert all(0 <= i < W and 0 <= j < H for i, j in texels) and sum(weights) == 65536
        for xs, ys in ((-1, 0), (0, -1), (xm + 1, 0), (0, ym + 1)):
            assert B.footprint(xs, ys, W, H) is None
    # through accumulate: a vertex on the last texel's centre gets that texel (an index past the image's end would raise)
    W, H = 2, 2
    image = B.noise_image(W, H, 2)
    state = B.accumulate(B.new_state(1), [B.pixel(256, 256, 1.0, W, H)], None, R.crafted_camera(W, H), image, None, W, H)
    assert state["sums"][0] == [65536 * int(image[1, 1, ch]) for ch in range(3)] + [256]


@pytest.mark.parametrize("name", sorted(B.EXPECT))
def test_the_crafted_cases_hit_what_they_are_crafted_for(name):
    out = B.expected(name)
    for k, n in B.EXPECT[name].items():
        assert out["totalsBeforeResolve"][k] == n, (name, k, out["totalsBeforeResolve"])


def test_the_weight_rule_case():
    m = B.case("weight-rule")
    out = B.expected("weight-rule")
    cam = m["views"][0]["camera"]
    c0 = B.cosine(cam, m["vertices"][0], m["normals"][0])
    assert F32(m["views"][0]["min_cos"]) == c0 and F32(m["views"][1]["min_cos"]) == np.nextafter(c0, F32(2))
    assert B.weight(cam, m["vertices"][0], m["normals"][0], m["views"][0]["min_cos"]) > 0, "a cosine equal to min_cos passes"
    assert B.weight(cam, m["vertices"][0], m["normals"][0], m["views"][1]["min_cos"]) == 0, "one ulp below min_cos does not"
    assert B.cosine(cam, m["vertices"][1], m["normals"][1]) > F32(1), "a cosine above 1 by rounding"
    assert B.weight(cam, m["vertices"][1], m["normals"][1], 1.0) == 256, "... is taken as 1"
    assert out["views"].tolist() == [2, 4, 0, 0, 0, 0, 0, 1], "equal and above: vertex 0; every view: vertex 1; back-facing, zero, NaN, Q = 0: none; Q = 2: min_cos 0 only"
    assert out["sums"][7, 3] == 2 and out["sums"][1, 3] == 4 * 256


def test_resolve_thresholds_and_fallback():
    state = B.new_state(4)
    state["sums"] = [[256 * 10 * 300, 256 * 20 * 300, 256 * 30 * 300, 300], [0, 0, 0, 0], [65280 * 7, 0, 128 * 7 - 1, 7], [128 * 7, 0, 0, 7]]
    state["views"] = [2, 0, 1, 1]
    fallback = np.arange(16, dtype=np.uint8).reshape(4, 4)
    colours, baked = B.resolve(state, fallback)
    assert baked.tolist() == [True, False, True, True] and state["totals"]["bakedVertices"] == 3
    assert colours.tolist() == [[10, 20, 30, 255], [4, 5, 6, 7], [255, 0, 0, 255], [1, 0, 0, 255]], "rounds to nearest, halves up; the largest sum gives 255"
    for kw, want in ((dict(min_views=2), [True, False, False, False]), (dict(min_views=3), [False] * 4), (dict(min_weight=7), [True, False, True, True]),
                     (dict(min_weight=8), [True, False, False, False]), (dict(min_views=0, min_weight=0), [True, False, True, True])):
        assert B.resolve(state, None, **kw)[1].tolist() == want, kw
    assert B.resolve(state)[0][1].tolist() == [0, 0, 0, 0], "no fallback: zeros"


def test_viewport_mismatch_accumulates_nothing():
    out = B.expected("viewport-mismatch")
    assert out["totals"]["viewportMismatch"] == 1 and out["views"].tolist() == [1, 1], "the second view alone is taken"
