"""CPU: the camera zoo (tests/camzoo.py) on the oracle alone.  First the conditions: every case reaches what it is there for -- nine non-zero rotation
entries, enough visible Gaussians, Gaussians behind and close to the camera, a tile list past the sort's 2 048-entry route, nothing visible at all, a
gradient that leaves the fp16 range -- so tests/test_gpu_cameras.py cannot pass vacuously.  The floors are about half of what was measured.  Then the
oracle itself under these cameras against float64: K1 against tests/indep64.py, K17 against central differences (tests/test_oracle_independent.py's
checks, tolerances unchanged), so that a difference found on the GPU is the kernel's."""
import functools

import numpy as np
import pytest

import camzoo
import indep64 as ind
import normal64 as n64
from test_oracle_independent import check_k1, check_k17

ROTATED = ("roll37", "side", "behind", "inside", "far", "away")           # nine non-zero rotation entries
POPULATED = ("roll37", "roll90", "roll180", "side", "behind", "below")


@functools.lru_cache(maxsize=None)
def _forward(name):
    from oracle import oracle as orc
    g, sh = camzoo.scene()
    st, ti = camzoo.settings()
    return orc.forward(g, sh, camzoo.camera(name), st, ti)


def _visible(name):
    return _forward(name)["tile_counts"] > 0


def _view_z(name):
    g, _ = camzoo.scene()
    cp = ind.camera_parts(camzoo.camera(name))
    return (ind.unpack_gaussians(g)["pos"] @ cp["rot"].T + cp["view"][:3, 3])[:, 2]


def _list_lengths(name):
    fw = _forward(name)
    return np.bincount(fw["sorted_keys"][:fw["total_entries"]] >> 16, minlength=2)


@pytest.mark.parametrize("name", camzoo.NAMES)
def test_every_matrix_is_a_rotation_and_the_block_holds_it(name):
    view = camzoo.view_matrix(name)
    R = view[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.norm(R @ R.T - np.eye(3)) < 1e-12
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    position = np.asarray(camzoo.poses()[name][0], np.float64)
    assert np.abs(view[:3, 3] + R @ position).max() < 1e-12 and np.array_equal(view[3], [0, 0, 0, 1])
    cam = camzoo.camera(name)
    assert np.array_equal(cam[0:16].reshape(4, 4).T, view.astype(np.float32))
    print(f"{name}: min |R_ij| = {np.abs(R).min():.3f}")
    if name in ROTATED:
        assert np.abs(R).min() >= 0.01, np.abs(R).min()


def test_look_at_without_roll_is_the_circle_camera():
    from webdgs_amd import synth
    cfg = camzoo.ZOO_CFG
    for i, blk in enumerate(synth.circle_cameras(cfg, 5, radius=1.5)):
        th = 2.0 * np.pi * i / 5
        view = camzoo.look_at((1.5 * np.cos(th), 1.5 * np.sin(th), 0.0), (0.0, 0.0, 6.0))
        assert np.array_equal(synth.camera_block(view, cfg.width, cfg.height, cfg.fy), blk)
    # a roll of 90 degrees: x' = y, y' = -x, the optical axis as it was
    a, b = camzoo.look_at((0.3, 0.2, 0), (0, 0, 6)), camzoo.look_at((0.3, 0.2, 0), (0, 0, 6), roll_deg=90.0)
    assert np.allclose(b[0, :3], a[1, :3], atol=1e-15) and np.allclose(b[1, :3], -a[0, :3], atol=1e-15) and np.array_equal(b[2], a[2])


@pytest.mark.parametrize("name", camzoo.NAMES)
def test_populations(name):
    fw = _forward(name)
    vis, z, lens = _visible(name), _view_z(name), _list_lengths(name)
    print(f"{name}: visible {int(vis.sum())} / tile entries {fw['total_entries']}, behind the camera {int((z < 0).sum())}, "
          f"visible at view z < 1: {int((vis & (z < 1)).sum())}, longest tile list {int(lens.max()) if fw['total_entries'] else 0}")
    if name in POPULATED:
        assert vis.sum() >= 2000
    if name == "inside":
        assert (z < 0).sum() >= 1000 and vis.sum() >= 100 and (vis & (z < 1)).sum() >= 5
    if name == "far":
        assert vis.sum() == camzoo.ZOO_CFG.num_points
        assert lens.max() > 2048, "a tile list past the 2 048 entries the segment sort holds in LDS"
    if name == "away":
        assert vis.sum() == 0 and fw["total_entries"] == 0


def test_close_leaves_the_fp16_range_from_finite_inputs():
    from oracle import oracle as orc
    g0, sh0 = camzoo.scene()
    g, sh = g0.copy(), sh0.copy()
    cam, target = camzoo.camera("close"), camzoo.target("close")
    st, ti = camzoo.settings()
    assert np.isfinite(g.view(np.float16).astype(np.float32)).all() and np.isfinite(sh.view(np.float16).astype(np.float32)).all() and np.isfinite(cam).all()
    state = orc.unpack(g, sh)
    ref = orc.train_step(g, sh, state, cam, st, ti, target)
    vis = ref["tile_counts"] > 0
    bad_grad = ~np.isfinite(ref["gradients"].view(np.float16).reshape(-1, 16).astype(np.float32)).all(axis=1)
    bad_rows = ~np.isfinite(g.view(np.float16).reshape(-1, 12).astype(np.float32)).all(axis=1)
    print(f"close: visible {int(vis.sum())} / tile entries {ref['total_entries']}; after one step {int(bad_grad.sum())} non-finite packed-gradient rows, "
          f"{int(bad_rows.sum())} non-finite re-packed Gaussian rows")
    assert bad_grad.sum() >= 1


@pytest.mark.parametrize("name", camzoo.NAMES)
def test_normals_near_the_flip_are_rare(name):
    g, _ = camzoo.scene()
    ref = n64.gaussian_normals64(g, camzoo.camera(name))
    near_flip = ref["valid"] & (np.abs(ref["facing"]) < n64.NEAR_FLIP)
    print(f"{name}: near_flip {near_flip.mean():.4%}")
    assert ref["valid"].all() and near_flip.mean() <= 0.005


@pytest.mark.parametrize("name", [n for n in camzoo.NAMES if n != "away"])
def test_k1_under_the_zoo(orc, name):
    g, sh = camzoo.scene()
    check_k1(orc, camzoo.ZOO_CFG, g, sh, camzoo.camera(name), population_floor=0.03 if name in ("inside", "close") else 0.3)


@pytest.mark.parametrize("name", [n for n in camzoo.NAMES if n != "away"])
def test_k17_under_the_zoo(orc, name):
    g, sh = camzoo.scene()
    check_k17(orc, camzoo.ZOO_CFG, g, sh, camzoo.camera(name))
