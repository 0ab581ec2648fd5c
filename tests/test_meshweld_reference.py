"""The welding restatement (tests/meshweld_ref.py: a stable sort on (key, slot) and a loop) against ``ops.weldTriangles`` (numpy's unique) on every crafted
soup, and its invariance under a permutation of the triangles.  No GPU."""
import numpy as np
import pytest

from webdgs_amd import ops

import meshweld_ref as W
from harness import assert_bits_equal

KEYS = ("vertices", "faces", "colours", "keys")


def _assert_same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype, f"{what}: {k} is {got[k].dtype}"
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_restatement_equals_weld_triangles(name):
    tri = W.case(name)
    got, want = W.weld(tri), ops.weldTriangles(tri)
    _assert_same(got, want, name)
    S = tri["keys"].size
    assert got["faces"].shape == (S // 3, 3) and got["keys"].shape[0] == np.unique(tri["keys"]).size
    if S:
        assert np.all(got["keys"][1:] > got["keys"][:-1])
        assert_bits_equal(got["keys"][got["faces"]], tri["keys"], f"{name}: every slot's rank names its key")


def test_lowest_slot_rule_on_unequal_payloads():
    tri = W.case("lowest-slot")
    got = W.weld(tri)
    keys = tri["keys"].reshape(-1)
    first = np.array([np.flatnonzero(keys == k)[0] for k in got["keys"]])
    assert got["keys"].size == 4 and np.array_equal(got["vertices"], np.repeat(first.astype(np.float32), 3).reshape(4, 3))
    assert np.array_equal(got["colours"], tri["colours"].reshape(-1, 4)[first, :3])
    # a soup without colours
    bare = dict(keys=tri["keys"], positions=tri["positions"], colours=None)
    assert W.weld(bare)["colours"] is None and ops.weldTriangles(bare)["colours"] is None


@pytest.mark.parametrize("name", ["extremes", "random-u64", "lowest-slot"])
def test_face_to_key_relation_is_invariant_under_a_permutation_of_the_triangles(name):
    tri = W.case(name)
    F = tri["keys"].shape[0]
    perm = np.random.default_rng(11).permutation(F)
    moved = {k: np.ascontiguousarray(v[perm]) for k, v in tri.items()}
    a, b = W.weld(tri), W.weld(moved)
    assert_bits_equal(b["keys"], a["keys"], f"{name}: the distinct keys")
    assert_bits_equal(b["keys"][b["faces"]], a["keys"][a["faces"]][perm], f"{name}: the keys the faces name")
    _assert_same(b, ops.weldTriangles(moved), f"{name}, permuted")


def test_pass_counts_of_the_crafted_cases():
    """What the GPU tests expect of the pass skipping, from the keys alone: a radix pass runs when its byte differs somewhere."""
    for name, want in W.PASSES_RUN.items():
        k = W.case(name)["keys"].reshape(-1)
        differs = int(np.bitwise_or.reduce(k) ^ np.bitwise_and.reduce(k)) if k.size else 0
        assert sum(1 for b in range(8) if (differs >> (8 * b)) & 255) == want, name
