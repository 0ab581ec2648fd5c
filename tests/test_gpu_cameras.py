"""GPU: the kernels that read the camera block -- project.hip (project_one: project_count_kernel, project_count_views_kernel), backward.hip (the
geometry kernels, the fused and the fp32 Adam behind them), normal.hip (the per-Gaussian normal) -- under the camera zoo of tests/camzoo.py: rotations
with nine non-zero entries, rolls of 90 and 180 degrees, a camera inside the cloud, one so far away that every splat is sub-pixel, one that sees
nothing, and one so close to a Gaussian that a gradient leaves the fp16 range.  Every other operator-level comparison in the suite runs under the
identity (exact products, a matrix that is its own transpose, the camera at the origin) or under an unrolled circle camera (view[0][1] == 0).

Bit for bit against the oracle, which tests/test_camera_zoo_reference.py pins to float64 under the same cameras; the normals and the composited
images against their float64 restatements within the bounds tests/test_gpu_normal.py and tests/test_gpu_depth.py state."""
import numpy as np
import pytest

from webdgs_amd import ops
from webdgs_amd.trainer import Trainer

import camzoo
import harness
import normal64 as n64
from harness import assert_bits_equal
from test_gpu_depth import _assert_depth_images_match_float64
from test_gpu_nan import step_differences
from test_gpu_normal import _assert_image_matches_float64, _assert_weight_channel, _assert_words_match_float64, _normals
from test_gpu_trainer_oracle import _compare

pytestmark = pytest.mark.gpu

CFG = camzoo.ZOO_CFG


def _scene():
    g, sh = camzoo.scene()
    return g.copy(), sh.copy()


# ---------------------------------------------------------------- a. two training steps, stage by stage
@pytest.mark.parametrize("name", camzoo.NAMES)
def test_two_steps_equal_the_oracle_stage_by_stage(hip_device, orc, name):
    g, sh = _scene()
    cam, target = camzoo.camera(name), camzoo.target(name)
    seen = []

    def make(dev, cfg, g_, sh_, cam_):
        seen.append(harness.HipPipeline(dev, cfg, g_, sh_, cam_))
        return seen[0]

    diffs = step_differences(orc, hip_device, CFG, g, sh, cam, target, steps=2, pipeline_factory=make, keep=True)
    pipe = seen[0]
    try:
        assert not diffs, "\n".join(diffs)
        if name == "away":   # nothing visible: no tile entry, and neither the cloud nor the optimizer state moves
            g0, sh0 = camzoo.scene()
            assert int(pipe.collect_forward()["stats"][0]) == 0
            assert_bits_equal(pipe.pc.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6)[:CFG.num_points], g0, "away: the cloud")
            assert_bits_equal(pipe.pc.sh_buffer.read(np.uint32).reshape(-1, 24)[:CFG.num_points], sh0, "away: the SH rows")
            fresh, state = orc.unpack(g0.copy(), sh0.copy()), pipe.read_state()
            for k in fresh:
                assert_bits_equal(state[k], fresh[k], f"away: optimizer state {k}")
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- b. the view-batched kernels
BATCHES = ([0, 3, 6, 1], [7, 2, 5, 4], [6, 6, 0, 7])


@pytest.mark.parametrize("batch_views", [True, False], ids=["view-batched-K1-K17", "per-view-kernels"])
def test_batched_steps_over_the_zoo_equal_the_oracle_trainer(hip_device, orc, batch_views):
    """Four views per step out of the eight populated zoo cameras: project_count_views_kernel and geometry_backward_views_kernel read four different
    camera blocks in one launch (or, per view, the per-view kernels add into the fp32 block), adam_repack_f32_kernel follows.  The oracle trainer's
    batched step with world = 1 sums the views' unpacked gradients in fp32 in view order, as the product does."""
    from oracle import oracle_trainer
    dev = hip_device
    g, sh = _scene()
    cams = [camzoo.camera(n) for n in camzoo.BATCH_NAMES]
    imgs = [camzoo.target(n) for n in camzoo.BATCH_NAMES]
    cameras = [dict(camera=c, width=CFG.width, height=CFG.height) for c in cams]
    images = [dict(texture=dev.bufferFrom(i), width=CFG.width, height=CFG.height) for i in imgs]
    o = oracle_trainer.OracleTrainer(g, sh, CFG.sh_deg, cams, imgs, densify=dict(schedule=dict(enabled=False)))
    t = Trainer(dev, seed=0, world_size=1, rank=0, views_per_rank=4, batch_views=batch_views)
    try:
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.setPointCloud(ops.createPointCloud(dev, g, sh, CFG.sh_deg))
        t.setDataset(cameras, images)
        t.start()
        assert t.batch_views is batch_views
        for i, batch in enumerate(BATCHES):
            o.step(batch, world=1)
            t.step(batch)
            _compare(t, o, f"after step {i + 1} on the views {[camzoo.BATCH_NAMES[v] for v in batch]}")
        g0, _ = camzoo.scene()
        assert not np.array_equal(o.g, g0), "training moved the cloud"
    finally:
        t.destroy()
        for im in images:
            im["texture"].destroy()


def test_single_view_steps_over_the_zoo_equal_the_oracle_trainer(hip_device, orc):
    """One view per step: the Trainer's own step, in which K17, Adam and the re-pack are one kernel that reads the camera block (the operator-level
    test above runs them as the reference's three).  Every populated zoo camera once, then two of them again, from their recorded command buffers."""
    from oracle import oracle_trainer
    dev = hip_device
    g, sh = _scene()
    cams = [camzoo.camera(n) for n in camzoo.BATCH_NAMES]
    imgs = [camzoo.target(n) for n in camzoo.BATCH_NAMES]
    cameras = [dict(camera=c, width=CFG.width, height=CFG.height) for c in cams]
    images = [dict(texture=dev.bufferFrom(i), width=CFG.width, height=CFG.height) for i in imgs]
    o = oracle_trainer.OracleTrainer(g, sh, CFG.sh_deg, cams, imgs, densify=dict(schedule=dict(enabled=False)))
    t = Trainer(dev, seed=0)
    try:
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.setPointCloud(ops.createPointCloud(dev, g, sh, CFG.sh_deg))
        t.setDataset(cameras, images)
        t.start()
        assert t.fuse_geometry_adam
        for i, v in enumerate(list(range(len(cams))) + [3, 6]):
            o.step(v)
            t.step([v])
            _compare(t, o, f"after step {i + 1} on the view {camzoo.BATCH_NAMES[v]}")
    finally:
        t.destroy()
        for im in images:
            im["texture"].destroy()


# ---------------------------------------------------------------- c. the per-Gaussian normals
@pytest.mark.parametrize("name", camzoo.NAMES)
def test_gaussian_normals_match_float64(hip_device, name):
    g, sh = _scene()
    cam = camzoo.camera(name)
    pipe = harness.HipPipeline(hip_device, CFG, g, sh, cam)
    try:
        words, img = _normals(pipe)
        if name != "away":
            _assert_words_match_float64(words, g, cam, name)
        else:
            ref = n64.gaussian_normals64(g, cam)
            assert np.array_equal(words == np.uint32(n64.NO_NORMAL), ~ref["valid"]), "away: which Gaussians have no normal"
            fw = pipe.collect_forward()
            assert fw["total_entries"] == 0 and not fw["tile_counts"].any() and fw["sorted_keys"].size == 0 and fw["sorted_values"].size == 0
            assert not fw["n_contrib"].any() and not fw["rgba8"][..., :3].any()
            assert np.all(img == 0), "away: no pixel has a weight or a normal"
    finally:
        pipe.destroy()


# ---------------------------------------------------------------- d. the composited images
@pytest.mark.parametrize("name", ["roll37", "inside", "far"])
def test_composited_normal_image_matches_float64(hip_device, name):
    g, sh = _scene()
    pipe = harness.HipPipeline(hip_device, CFG, g, sh, camzoo.camera(name))
    try:
        words, img = _normals(pipe)
        assert _assert_weight_channel(pipe, img, name) == 0
        n_active = _assert_image_matches_float64(pipe, words, img, name)
        assert int(n_active.max()) > 0
    finally:
        pipe.destroy()


@pytest.mark.parametrize("name", ["roll37", "inside", "far"])
def test_depth_images_match_float64(hip_device, name):
    g, sh = _scene()
    stats = _assert_depth_images_match_float64(hip_device, CFG, g, sh, camzoo.camera(name), name)
    assert int(stats["n_active"].max()) > 0
