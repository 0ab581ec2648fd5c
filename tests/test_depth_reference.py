"""The float64 restatement of the depth images (tests/depth64.py) against the parity oracle's forward stages, a hand-made scene with a known answer,
the presentation formula's tie share, and loaders.backprojectDepth.  No GPU: this protects the yardstick the GPU depth tests measure against."""
import functools
import math

import numpy as np
import pytest

from webdgs_amd import loaders, synth

import depth64 as d64
import harness

MASK_CAP = 0.005   # share of the image's pixels either exclusion mask may hold

# the first five are the CPU scenes; the sixth (c2 in full) is walked by the GPU tests only
SCENES = {
    "c1": dict(base="c1"),
    "c2-20k": dict(base="c2", num_points=20_000, width=320, height=240),
    "big-splats": dict(base="c1", num_points=3_000, width=97, height=61, sh_deg=2, s0=0.05),
    "odd-size": dict(base="c1", num_points=4_000, width=250, height=130),
    "sparse": dict(base="c1", num_points=300),
    "c2": dict(base="c2"),
}
CPU_SCENES = list(SCENES)[:5]


def scene_config(name):
    return harness.small_config(**SCENES[name])


def depth64_of(stages, cfg, max_entries=0, probe=None):
    """depth64 on the forward stages as oracle.forward / HipPipeline.collect_forward return them."""
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    stats = {}
    out = d64.depth64(st, ti, stages["splats"], stages["depths"], stages["tile_ranges"], stages["sorted_keys"], stages["sorted_values"],
                      stages["total_entries"], max_entries=max_entries, stats=stats, probe=probe)
    return out + (stats,)


@functools.lru_cache(maxsize=None)
def reference(name):
    from oracle import oracle as orc
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    ref = orc.forward(g, sh, cam, synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0))
    return cfg, ref, depth64_of(ref, cfg)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_weight_sum_is_the_oracles_transmittance(name):
    cfg, ref, (A, D, M, near_sat, near_half, stats) = reference(name)
    err = np.abs((1.0 - A) - ref["final_T"].astype(np.float64))
    print(f"{name}: E={ref['total_entries']} max|(1-A64)-final_T| = {err[~near_sat].max():.3g} near_sat {near_sat.mean():.4%} near_half {near_half.mean():.4%}")
    assert err[~near_sat].max() <= 1e-6


@pytest.mark.parametrize("name", CPU_SCENES)
def test_masks_and_ranges(name):
    cfg, ref, (A, D, M, near_sat, near_half, stats) = reference(name)
    assert near_sat.mean() <= MASK_CAP and near_half.mean() <= MASK_CAP, (near_sat.mean(), near_half.mean())
    covered = stats["n_active"] > 0
    # D is a convex combination of the active records' depths (float64 rounding of the sums: a few 1e-16 relative)
    slack = 1e-12 * np.where(covered, np.abs(stats["z_max"]), 0.0)
    assert np.all(D[covered] >= (stats["z_min"] - slack)[covered]) and np.all(D[covered] <= (stats["z_max"] + slack)[covered])
    assert np.all(D[~covered] == 0) and np.all(M[~covered] == 0) and np.all(A[~covered] == 0)
    assert np.all(A[covered] > 0) and np.all(D[covered] != 0)
    assert np.array_equal(M != 0, A >= 0.5)
    # M is the stored z of one of the pixel's records
    _, _, _, _, _, probed = depth64_of(ref, cfg, probe=M.astype(np.float32))
    assert np.all(probed["probe_in_box"][M != 0])
    assert np.all((M >= stats["z_min"])[M != 0]) and np.all((M <= stats["z_max"])[M != 0])
    if name == "sparse":
        assert 0.2 < covered.mean() < 0.5, "the sparse scene is there for its empty pixels"
    else:
        assert covered.all()


def _two_gaussians(o1, o2, z1=2.0, z2=4.0):
    """Two Gaussians whose centres project exactly onto the centre of pixel (32, 32) of a 64 x 64 image: fy = 32 makes the projection's scale 1, and
    x = y = z / 64 (fp16-exact) gives ndc 1/64, pixel coordinate 32.5.  dx = dy = 0 there, so alpha is the opacity the Splat stores."""
    cfg = harness.small_config("c1", num_points=2, width=64, height=64, sh_deg=0, fy=32.0)
    g = np.zeros((2, 12), np.float16)
    for i, (z, o) in enumerate(((z1, o1), (z2, o2))):
        g[i, 0:4] = [z / 64.0, z / 64.0, z, o]
        g[i, 4] = 1.0
        g[i, 8:11] = math.log(0.05 * z)
    sh = np.zeros((2, 48), np.float16)
    sh[:, 0:3] = 0.5
    return cfg, g.view(np.uint32).reshape(2, 6), sh.view(np.uint32).reshape(2, 24), synth.identity_camera(cfg)


@pytest.mark.parametrize("o1,front_wins", [(-1.0, False), (0.0, True), (1.0, True)])
def test_two_gaussians_on_one_pixel(o1, front_wins):
    from oracle import oracle as orc
    z1, z2, o2 = 2.0, 4.0, 3.0
    cfg, g, sh, cam = _two_gaussians(o1, o2, z1, z2)
    ref = orc.forward(g, sh, cam, synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0))
    assert ref["total_entries"] >= 2
    A, D, M, _, _, stats = depth64_of(ref, cfg)
    # by hand: the opacities as fp16 (the Splat's storage), w1 = a1, w2 = a2 (1 - a1)
    a1 = float(np.float16(1.0 / (1.0 + math.exp(-o1))))
    a2 = float(np.float16(1.0 / (1.0 + math.exp(-o2))))
    stored = ref["splats"].view(np.uint16).reshape(-1, 12)[:, 11].view(np.float16).astype(np.float64)
    assert stored[0] == a1 and stored[1] == a2, stored
    assert np.array_equal(d64.decode_depths(ref["depths"]), np.array([z1, z2], np.float32))
    w1, w2 = a1, a2 * (1.0 - a1)
    assert stats["n_active"][32, 32] == 2
    assert A[32, 32] == pytest.approx(w1 + w2, rel=1e-15)
    assert D[32, 32] == pytest.approx((w1 * z1 + w2 * z2) / (w1 + w2), rel=1e-15)
    assert M[32, 32] == (z1 if front_wins else z2)
    assert (a1 >= 0.5) == front_wins


@pytest.mark.parametrize("name", CPU_SCENES)
def test_presentation_formula_ties_are_rare(name):
    """Pixels whose float64 255 t lies within 1e-3 of a .5 tie -- where an implementation of the formula may round to the other neighbour -- stay under
    0.5 % of the image on the scenes' own expected-depth images."""
    cfg, ref, (A, D, M, near_sat, near_half, stats) = reference(name)
    d = D.astype(np.float32)
    near, far = d[d > 0].min(), d[d > 0].max()
    grey, v = d64.depth_to_rgba8_64(d, near, far)
    ties = np.abs((v - np.floor(v)) - 0.5) < 1e-3
    print(f"{name}: tie share {ties.mean():.4%}")
    assert ties.mean() <= 0.005
    assert np.all(grey[d == 0] == 0) and grey.max() == 255


def test_backproject_depth_inverts_the_projection():
    cfg = harness.small_config("c1", num_points=1, width=97, height=61)
    cam = synth.circle_cameras(cfg, 8)[3]
    depth = np.full((cfg.height, cfg.width), 3.25, np.float32)
    depth[5, 7] = 0.0   # no depth: no point
    pts = loaders.backprojectDepth(depth, cam)
    assert pts.dtype == np.float32 and pts.shape == (cfg.width * cfg.height - 1, 3)
    ys, xs = np.nonzero(depth > 0)
    blk = cam.astype(np.float64)
    view = blk[0:16].reshape(4, 4).T
    v = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], axis=1) @ view.T
    # Bound.  The point is V^-1 v evaluated in float64 and stored as float32: each coordinate is off by at most 2^-24 |P|.  The block's inverse view
    # matrix is itself a float32 rounding of the inverse (each entry off by 2^-24 of its size), so V V^-1 differs from the identity by at most
    # 4 * 2^-24 * max|V| max|V^-1| per entry.  Taking the point through V again multiplies both by at most 4 max|V| (four terms per row).  With
    # m = max(1, max|V|, max|V^-1|) and s = max(|v|, |P|) that is |v' - v| <= (4 m * 1 + 4 * 4 m^2) 2^-24 s <= 20 m^2 2^-24 s per coordinate.
    m = max(1.0, np.abs(view).max(), np.abs(blk[16:32]).max())
    s = max(np.abs(v[:, :3]).max(), np.abs(pts).max())
    bound = 20.0 * m * m * 2.0 ** -24 * s
    assert np.abs(v[:, 2] - depth[ys, xs]).max() <= bound, (np.abs(v[:, 2] - depth[ys, xs]).max(), bound)
    # pixel = (P00 x / z / 2 + 1/2) W: an error e in x and in z moves it by at most W P00 / 2 * (e / z + |x| e / z^2) <= W P00 e (1 + |x| / z) / (2 z)
    p00, p11 = blk[32], blk[37]
    pix_x = (p00 * v[:, 0] / v[:, 2] * 0.5 + 0.5) * cfg.width
    pix_y = (p11 * v[:, 1] / v[:, 2] * -0.5 + 0.5) * cfg.height
    zmin = v[:, 2].min()
    reach = 1.0 + max(np.abs(v[:, 0]).max(), np.abs(v[:, 1]).max()) / zmin
    bx = cfg.width * abs(p00) * bound * reach / (2.0 * zmin) + 97 * 2.0 ** -50   # (+ the float64 evaluation of the expectation itself)
    by = cfg.height * abs(p11) * bound * reach / (2.0 * zmin) + 97 * 2.0 ** -50
    assert np.abs(pix_x - (xs + 0.5)).max() <= bx and np.abs(pix_y - (ys + 0.5)).max() <= by
    with pytest.raises(ValueError):
        loaders.backprojectDepth(np.zeros(5, np.float32), cam)
