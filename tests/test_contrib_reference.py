"""The float64 restatement of the per-Gaussian contribution (tests/contrib64.py) against the parity oracle's forward stages and depth64, a hand-made scene
with a known answer, and the conditions that keep the restatement's slack from hiding a failure.  No GPU: this protects the yardstick the GPU contribution
tests measure against."""
import functools
import math

import numpy as np
import pytest

from webdgs_amd import synth

import contrib64 as c64
import depth64 as d64
from test_depth_reference import _two_gaussians, reference

SCENES = ["sparse", "c1", "c2-20k", "big-splats"]


def contrib64_of(stages, cfg, max_entries=0):
    """contrib64 on the forward stages as oracle.forward / HipPipeline.collect_forward return them."""
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    return c64.contrib64(st, ti, stages["splats"], stages["tile_ranges"], stages["sorted_keys"], stages["sorted_values"], stages["total_entries"],
                         max_entries=max_entries)


@functools.lru_cache(maxsize=None)
def contribution(name):
    cfg, ref, depth = reference(name)
    return cfg, ref, depth, contrib64_of(ref, cfg)


@pytest.mark.parametrize("name", SCENES)
def test_weights_are_the_images_weights(name):
    cfg, ref, (A, D, M, near_sat, near_half, stats), c = contribution(name)
    total_g, total_p = c["weight_sum"].sum(), A.sum()
    print(f"{name}: sum_g weight_sum = {total_g:.6f}, sum_p A64 = {total_p:.6f}, relative difference {abs(total_g - total_p) / total_p:.3g}")
    assert abs(total_g - total_p) <= 1e-9 * total_p
    assert np.array_equal(c["A"], A)
    assert int(c["pixels"].sum()) == int(stats["n_active"].sum())
    assert c["max_weight"].max() <= d64.F99
    assert np.all(c["max_weight"] <= c["weight_sum"] + 1e-300) and np.all((c["pixels"] == 0) == (c["weight_sum"] == 0))
    assert not np.any(c["surely_zero"] & (c["pixels"] > 0))


@pytest.mark.parametrize("name", SCENES)
def test_slack_cannot_hide_a_failure(name):
    cfg, ref, depth, c = contribution(name)
    slack, weight = c["slack_sum"].sum(), c["weight_sum"].sum()
    print(f"{name}: slack {slack:.4g} on {weight:.6g} ({slack / weight:.3%}) on {int((c['slack_sum'] > 0).sum())} of {len(c['slack_sum'])} Gaussians, "
          f"worst single {c['slack_sum'].max():.3g}; surely_zero {int(c['surely_zero'].sum())}, non-zero weight_sum {int((c['weight_sum'] > 0).sum())}")
    if name in ("sparse", "c1"):
        assert slack == 0 and c["slack_pixels"].sum() == 0 and c["slack_max"].max() == 0
    else:
        assert slack <= 0.005 * weight
    if name == "big-splats":
        assert c["surely_zero"].sum() >= 500
        assert (c["weight_sum"] > 0).sum() <= 100


@pytest.mark.parametrize("o1", [-1.0, 0.0, 1.0])
def test_two_gaussians_on_one_pixel(o1):
    from oracle import oracle as orc
    o2 = 3.0
    cfg, g, sh, cam = _two_gaussians(o1, o2)
    ref = orc.forward(g, sh, cam, synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0))
    c = contrib64_of(ref, cfg)
    a1 = float(np.float16(1.0 / (1.0 + math.exp(-o1))))
    a2 = float(np.float16(1.0 / (1.0 + math.exp(-o2))))
    # dx = dy = 0 at pixel (32, 32): alpha is the stored opacity, the largest the Gaussian reaches anywhere; the front one is composited onto A = 0
    assert c["max_weight"][0] == a1
    assert c["max_weight"][1] >= a2 * (1.0 - a1)   # (the back one's largest weight may lie where the front one is fainter)
    assert c["max_weight"][1] <= a2
    assert c["pixels"][0] > 0 and c["pixels"][1] > 0 and c["slack_sum"].sum() == 0
