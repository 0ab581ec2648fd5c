"""CPU: the restatement of per-face visibility, its rule and the face filter (tests/meshvisibility_ref.py): the sums it must keep, its indifference to the
order of the pixels, the rule's fixed-point comparison at exact equality, the host form of the rule (``ops.selectFaces``) against the restatement's loop, and
the filter under an all-ones mask against the keep-everything compaction of tests/meshclean_ref.py."""
import numpy as np
import pytest

from webdgs_amd import ops

import meshclean_ref as M
import meshvisibility_ref as VR


def _depths(n, seed):
    """Mesh depth, model depth and weight sum for n pixels: mostly close pairs, with absent, non-finite and negative values mixed in."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(1.0, 5.0, n).astype(np.float32)
    b = (a + rng.uniform(-0.1, 0.1, n).astype(np.float32)).astype(np.float32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    kind = rng.integers(0, 12, n)
    for k, (arr, value) in enumerate(((a, 0.0), (b, 0.0), (b, np.nan), (b, np.inf), (b, -1.0), (a, np.inf))):
        arr[kind == k] = value
    return a, b, w


@pytest.mark.parametrize("name", sorted(VR.IMAGES))
def test_sums_of_one_view(name):
    F, w, h, img = VR.image(name)
    a, b, ws = _depths(img.size, 3)
    acc = VR.Accumulator(F)
    counted, agreeing, foreign = acc.accumulate(img, a, b, ws, 0.5, 0.05)
    c = acc.counters.astype(np.int64)
    assert c.shape == (F, 3)
    assert int(c[:, 0].sum()) == counted == int(np.sum(img.astype(np.int64) < F))
    assert int(c[:, 1].sum()) == agreeing and np.all(c[:, 1] <= c[:, 0])
    assert np.array_equal(c[:, 2], (c[:, 0] > 0).astype(np.int64))
    assert counted + foreign + int(np.sum(img == VR.EMPTY)) == img.size
    assert acc.stats() == dict(views=1, foreignPixels=foreign, countedPixels=counted, agreeingPixels=agreeing)
    # without depth images every counted pixel agrees
    plain = VR.Accumulator(F)
    plain.accumulate(img)
    assert np.array_equal(plain.counters[:, 1], plain.counters[:, 0]) and np.array_equal(plain.counters[:, 0], acc.counters[:, 0])


def test_images_are_what_the_issue_describes():
    assert VR.image("one-face-67x45")[3].size % 2 == 1 and VR.image("one-face-67x45")[3].size % 256 != 0
    F, w, h, img = VR.image("run-lengths")
    edges = np.flatnonzero(np.diff(img.astype(np.int64)) != 0) + 1
    assert np.array_equal(np.diff(np.concatenate([[0], edges, [img.size]])), np.arange(1, 131))
    F, w, h, img = VR.image("alternating")
    assert np.all(img[1:] != img[:-1]) and set(img.tolist()) == {0, 1}
    F, w, h, img = VR.image("foreign")
    for value in (F, 2 ** 31, 0xFFFFFFFE, VR.EMPTY):
        assert np.any(img == value)
    assert VR.image("random-100000")[0] == 100000 and VR.image("no-faces")[0] == 0


def test_views_count_calls_that_show_the_face():
    acc = VR.Accumulator(4)
    first, second, third = np.array([0, 0, 1, VR.EMPTY], np.uint32), np.array([1, 1, 1, 2], np.uint32), np.array([0, 3, 7, 1], np.uint32)
    for img in (first, second, third):
        acc.accumulate(img)
    assert acc.counters.tolist() == [[3, 3, 2], [5, 5, 3], [1, 1, 1], [1, 1, 1]]   # face 0: calls 1 and 3 only
    assert np.all(acc.counters[:, 2] <= acc.views) and acc.views == 3 and acc.foreign == 1


@pytest.mark.parametrize("name", ["run-lengths", "random-5", "foreign"])
def test_a_permutation_of_the_pixels_changes_nothing(name):
    F, w, h, img = VR.image(name)
    a, b, ws = _depths(img.size, 5)
    order = np.random.default_rng(29).permutation(img.size)
    one, two = VR.Accumulator(F), VR.Accumulator(F)
    one.accumulate(img, a, b, ws, 0.5, 0.05)
    two.accumulate(img[order], a[order], b[order], ws[order], 0.5, 0.05)
    assert np.array_equal(one.counters, two.counters) and one.stats() == two.stats()


def test_agreement_is_depth_agreements_presence_rule_in_f32():
    t = np.float32(0.0625)   # (a power of two: 2 + t and the ulp above it differ from 2 by f32 values exactly)
    a = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0], np.float32)
    over = np.nextafter(np.float32(2.0) + t, np.float32(np.inf))
    b = np.array([0.0, np.nan, np.inf, -1.0, np.float32(2.0) + t, over, 2.0, 2.0, 2.0, 2.0], np.float32)
    assert np.float32(b[4] - a[4]) == t < np.float32(b[5] - a[5])   # the difference equal to the threshold, and one ulp over
    w = np.array([1, 1, 1, 1, 1, 1, 1, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, 1], np.float32)
    assert VR.agrees(a, b, w, 0.5, t).tolist() == [False, False, False, False, True, False, False, False, True, True]
    assert VR.agrees(a, b, None, 0.5, t).tolist() == [False, False, False, False, True, False, False, True, True, True]


def test_the_overflow_rule_is_host_arithmetic():
    acc = VR.Accumulator(1)
    assert not acc.would_overflow(8192, 8192)
    acc.views = 62
    assert not acc.would_overflow(8192, 8192)   # 63 2^26 < 2^32
    acc.views = 63
    assert acc.would_overflow(8192, 8192) and not acc.would_overflow(8192, 8191) and not acc.would_overflow(1, 1)


def test_rule_at_exact_equality():
    counters = np.array([[10, 5, 2], [10, 4, 2], [0, 0, 0], [3, 1, 1], [65536, 21845, 1], [65536, 21846, 1], [2 ** 32 - 1, 2 ** 32 - 1, 7]], np.uint32)
    half = VR.fraction_q16(0.5)
    assert half == 32768 and VR.fraction_q16(1.0) == 65536 and VR.fraction_q16(0.0) == 0
    assert VR.flags(counters, 0, 0, 0, half).tolist() == [1, 0, 1, 0, 0, 0, 1]       # 5 / 10 is one half exactly; a face without pixels passes the fraction
    assert VR.flags(counters, 1, 0, 0, half).tolist() == [1, 0, 0, 0, 0, 0, 1]
    third = VR.fraction_q16(1.0 / 3.0)
    assert third == 21845                                                            # rint(21845.33)
    assert VR.flags(counters, 1, 0, 0, third).tolist() == [1, 1, 0, 1, 1, 1, 1]       # 21845 65536 = 21845 65536: equality keeps
    assert VR.flags(counters, 1, 0, 0, third + 1).tolist() == [1, 1, 0, 0, 0, 1, 1]   # 1 / 3 < 21846 / 65536; 21845 / 65536 < it too
    assert VR.flags(counters, 1, 0, 0, 65536).tolist() == [0, 0, 0, 0, 0, 0, 1]       # the products need 64 bits
    for name, at in (("min_pixels", 10), ("min_views", 2), ("min_agreeing", 5)):
        kw = dict(min_pixels=0, min_views=0, min_agreeing=0)
        assert VR.flags(counters[:1], **dict(kw, **{name: at})).tolist() == [1] and VR.flags(counters[:1], **dict(kw, **{name: at + 1})).tolist() == [0]


def test_select_faces_is_the_restatements_rule():
    rng = np.random.default_rng(41)
    pixels = rng.integers(0, 50, 4000)
    counters = np.stack([pixels, rng.integers(0, 51, 4000) * pixels // 50, rng.integers(0, 5, 4000)], axis=1).astype(np.uint32)
    counters[:3] = [[2 ** 32 - 1, 2 ** 32 - 1, 1], [2 ** 32 - 1, 2 ** 32 - 2, 1], [0, 0, 0]]
    for rule in (dict(), dict(minPixels=0), dict(minPixels=7, minViews=2), dict(minAgreeing=3), dict(minAgreeingFraction=0.5), dict(minAgreeingFraction=1.0),
                 dict(minPixels=2, minViews=1, minAgreeing=1, minAgreeingFraction=1.0 / 3.0)):
        got = ops.selectFaces(counters, **rule)
        want = VR.flags(counters, rule.get("minPixels", 1), rule.get("minViews", 1), rule.get("minAgreeing", 0), VR.fraction_q16(rule.get("minAgreeingFraction", 0.0)))
        assert got.dtype == bool and np.array_equal(got, want.astype(bool)), rule
    assert ops.selectFaces(np.zeros((0, 3), np.uint32)).shape == (0,)
    for bad in (dict(minAgreeingFraction=1.5), dict(minAgreeingFraction=-0.1), dict(minAgreeingFraction=float("nan")), dict(minPixels=-1), dict(minViews=2 ** 32)):
        with pytest.raises(Exception):
            ops.selectFaces(counters, **bad)


@pytest.mark.parametrize("name", ["clusters", "only-invalid", "no-faces", "no-vertices", "one-face", "bridge-first"])
def test_all_ones_is_the_keep_everything_compaction(name):
    faces, V, labels = M.shape(name)
    mesh = dict(M.as_mesh(faces, V), colours=np.random.default_rng(2).integers(0, 256, (V, 3)).astype(np.uint8), keys=np.arange(V, dtype=np.uint64) * np.uint64(3))
    want = M.compact(mesh, labels, np.ones(labels["count"], bool))
    got = VR.filter_faces(mesh, np.ones(faces.shape[0], np.uint8))
    for k in ("vertices", "faces", "vertexMap", "faceMap", "colours", "keys"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{name}: {k}"
    assert got["invalidFaces"] == labels["invalidFaces"]
    if name == "clusters":
        assert labels["invalidFaces"] > 0 and got["vertices"].shape[0] < V   # invalid faces and unreferenced vertices are what it is about


def test_filter_masks():
    faces, V, labels = M.shape("clusters")
    mesh = M.as_mesh(faces, V)
    none = VR.filter_faces(mesh, np.zeros(faces.shape[0], np.uint8))
    assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["invalidFaces"] == labels["invalidFaces"]
    valid = np.all(faces.astype(np.int64) < V, axis=1)
    only_invalid = VR.filter_faces(mesh, (~valid).astype(np.uint8))
    assert only_invalid["faces"].shape == (0, 3) and only_invalid["vertexMap"].size == 0
    keep = (np.arange(faces.shape[0]) % 2 == 0).astype(np.uint8) * 255   # any non-zero flag keeps
    got = VR.filter_faces(mesh, keep)
    assert np.array_equal(got["faceMap"], np.flatnonzero((keep != 0) & valid))
    assert np.array_equal(got["vertices"][got["faces"].astype(np.int64)], mesh["vertices"][faces[got["faceMap"]].astype(np.int64)])   # the same triangles
    assert np.all(np.diff(got["vertexMap"].astype(np.int64)) > 0) and np.array_equal(np.unique(got["faces"]), np.arange(got["vertexMap"].size))
    again = VR.filter_faces(got, np.ones(got["faces"].shape[0], np.uint8))
    assert np.array_equal(again["faces"], got["faces"]) and np.array_equal(again["vertices"], got["vertices"])   # a second pass reproduces the first
