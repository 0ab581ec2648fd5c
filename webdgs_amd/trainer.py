"""``Trainer`` -- counterpart of ``/root/reference/src/trainer.ts`` driving the HIP operator classes.

Public surface and sequencing follow the reference (method names as in ``trainer.ts:177-566``):
``step()`` = random view -> camera upload -> forward -> rasterize -> backward -> Adam -> submit+sync -> it/s EMA ->
scheduled ``runDensifyPruneMultiView()`` (``trainer.ts:568-660``, ``373-497``).  Divergences, all host-side and documented in
DESIGN.md: the rasterizer's grid always follows the current viewport (fixes SURVEY Q19); metric views each render with
their own camera (fixes Q12: uploads are stream-ordered here); the point-cloud swap is applied inside the step that
produced it instead of on the next animation frame.  New: ``world_size > 1`` runs view-sharded data parallelism
(``webdgs_amd.parallel``).

This class is the training step and what it needs.  Everything that measures the model without training it -- ``evaluate``, ``normalConsistency``,
``fuseDepth``, ``extractMesh``, ``evaluateGeometry``, ``contributionStats`` -- lives in ``evaluation.Evaluator``; the methods of those names here
delegate to it.  Every host wait goes through ``ops.CapacityReports.settle``, which sorts the device-wide capacity reports by owner.
"""
from __future__ import annotations

import dataclasses
import math
import os
import random
import time
import warnings
from typing import Optional

import numpy as np
import torch

from . import loaders, ops, parallel


@dataclasses.dataclass
class PassSet:
    """The passes that render one view at a time, and what they own between them.  A training set has all three passes; a metric set (one per
    metric lane of a densify event) has the metric pass as ``backwardPass``, its down-sampled ground truth as ``target`` and its camera block;
    an evaluation set has no backward pass."""
    forwardPass: ops.TiledForwardPass
    rasterizer: ops.TiledRasterizer
    backwardPass: Optional[ops.TiledBackwardPass] = None
    target: Optional[ops.HipBuffer] = None
    cameraBuffer: Optional[ops.HipBuffer] = None
    ownsCamera: bool = False   # (metric set 0 renders through the trainer's own ``metricsCameraBuffer``, which outlives it)

    def destroy(self) -> None:
        for owned in (self.forwardPass, self.rasterizer, self.backwardPass, self.target, self.cameraBuffer if self.ownsCamera else None):
            if owned is not None:
                owned.destroy()


def destroy_pass_sets(sets) -> None:
    """Destroys every pass of ``sets``, in set order."""
    for s in sets:
        s.destroy()


from . import evaluation  # noqa: E402  (it imports PassSet and destroy_pass_sets from here)


class Trainer:
    def __init__(self, device: ops.HipDevice, trainingConfig: Optional[dict] = None, seed: int = 0, world_size: int = 1, rank: int = 0,
                 views_per_rank: int = 1, maxTileEntries: int = 0, use_command_buffers: bool = True, exchange: Optional[parallel.Exchange] = None,
                 overlap_views: Optional[bool] = None, pipeline_depth: int = 1, batch_views: Optional[bool] = None):
        ops.dssim_mode(trainingConfig)   # (an unknown loss is refused before anything is built)
        self.device = device
        self.trainingConfig = dict(trainingConfig or dict(lambda_l1=0.8, lambda_l2=0.0, lambda_dssim=0.2))  # trainer.ts:100-104
        self.optimizerHyperparameters = dict(ops.DEFAULT_ADAM_HYPERPARAMETERS)
        self.world_size, self.rank, self.views_per_rank = int(world_size), int(rank), max(1, int(views_per_rank))
        self.maxTileEntries = int(maxTileEntries)
        self._grown_tile_entries = 0  # (auto sizing only: what an overflow has made of the lists, step())
        self._foreign_overflow_warned = False
        # the transport of the data-parallel exchange (parallel.Exchange); world_size == 1 needs none
        self.exchange = exchange if exchange is not None else (parallel.default_exchange(device, self.world_size) if self.world_size > 1 else parallel.Exchange())
        # sliced step (reduce-scatter / owned-slice Adam / all-gather): any real exchange, also a forced one in a world of one
        self._sliced = self.world_size > 1 or bool(getattr(self.exchange, "force", False))
        if self.world_size > 1 and (self.exchange.world_size, self.exchange.rank) != (self.world_size, self.rank):
            raise ValueError(f"exchange is rank {self.exchange.rank} of {self.exchange.world_size}, trainer is rank {self.rank} of {self.world_size}")
        # Recorded command buffers (HIP graphs), one per view set: the reference re-records its encoder every step; here the
        # recording is kept and re-submitted, because every size the kernels need is read on the device.
        self.use_command_buffers = bool(use_command_buffers)
        self._cmd_cache: dict = {}
        self._eager_steps = 0
        # A batched step deals its views to several op sets in turn; once their command buffers are recorded, set s replays on the
        # device's lane s, so the bandwidth-bound stages of one view (project, sort, loss, geometry backward) run beside the
        # VALU-bound rasterization kernels of another.  Results do not depend on it: the fp32 block is still filled in view order.
        # overlap_views: None = default (WDGS_LANES, else DEFAULT_LANES), False / 1 = one lane, True or n = that many lanes.
        if overlap_views is None:
            overlap_views = int(os.environ.get("WDGS_LANES", self.DEFAULT_LANES))
        elif isinstance(overlap_views, bool):
            overlap_views = self.DEFAULT_LANES if overlap_views else 1
        self._lanes = max(1, min(int(overlap_views), self.views_per_rank, ops.MAX_LANES))
        # View-batched kernels (round 3): a batched step projects every Gaussian for ALL its views in one launch (K1) and turns all the
        # views' accumulators into the step's fp32 gradient block in one launch (K17) -- Gaussian and SH row read once per step instead
        # of once per view, the fp32 block written once, and no cross-lane ordering of per-view K17s.  Every view then needs buffers of
        # its own: one op set per view of the batch (the lanes -- in-order streams -- stay at `_lanes`).  False (WDGS_BATCH_VIEWS=0): the
        # per-view kernels of round 2, one op set per lane.  The results are identical.
        self.batch_views = self.views_per_rank > 1 and (os.environ.get("WDGS_BATCH_VIEWS", "1") != "0" if batch_views is None else bool(batch_views))
        self._op_sets = min(self.views_per_rank, ops.MAX_BATCH_VIEWS) if self.batch_views else self._lanes
        # views per batched launch: 0 = all the step's views in one K1 and one K17 (measured best at c3, 8 views: 1875 views/s; groups of
        # 3 on their own lane, overlapping the other groups' rasterization, 1798: the batched kernels then re-read the cloud per group and
        # take issue slots from the VALU-bound rasterization kernels they run beside -- profiles/r03i_*)
        self.view_group = int(os.environ.get("WDGS_VIEW_GROUP", "0"))
        self._camera_buffers: list = []
        # every rank draws the same view sequence (same seed), then takes its shard
        self._rng = random.Random(seed)

        self._train_sets: list = []  # PassSet per op set of a step (set 0: the single-view step's, the public forwardPass / rasterizer / backwardPass)
        self.optimizer = None
        # pipeline_depth 1: every step awaits its own completion, as trainer.ts:639-645 does.  2: step() returns once the PREVIOUS
        # step has finished, so the host prepares and submits step k+1 while step k runs (the device never idles across the step
        # boundary); a capacity error then surfaces one step late -- the device-side guard has already kept that step's Adam from
        # running on incomplete gradients.  Densify steps, stop() and every read-back drain the pipeline first.
        self.pipeline_depth = max(1, min(int(pipeline_depth), 4))
        self.reuse_passes = True  # applyPointCloudSwap resizes the passes instead of rebuilding them (False: the reference's teardown)
        self.fuse_geometry_adam = True  # the single-view step runs K17, Adam and the re-pack as one kernel (False: the reference's three)
        self.keep_gradients = os.environ.get("WDGS_KEEP_GRADIENTS", "0") == "1"  # the fused step also fills backwardPass.getGradientsBuffer()
        # Adam writes the trained SH-DC halves to a compact array that K1 reads, instead of 6 bytes into every 96-byte SH row each step; the
        # rows are flushed at hand-over points (Optimizer.setDeferredSH).  False: the reference's write pattern.  Results are identical.
        self.deferred_sh = os.environ.get("WDGS_DEFERRED_SH", "1") != "0"
        self._dc_words: Optional[ops.HipBuffer] = None
        self._gradient_output_applied: Optional[bool] = None
        self._tickets: list = []
        self.metricsViewportWidth = self.metricsViewportHeight = 0
        # The metric views of a densify event are independent until normalizeMetricCounts (counts are integer atomics: any order gives the
        # same bits): they are dealt to `metric_lanes` op sets, each on a device lane of its own, all adding into set 0's counts
        # (TiledBackwardPass.setMetricCountsTarget).  The reference walks them one after the other through one pass (trainer.ts:391-430).
        self.metric_lanes = max(1, min(int(os.environ.get("WDGS_METRIC_LANES", self.DEFAULT_LANES)), ops.MAX_LANES))
        self._metric_sets: list = []  # PassSet per metric lane (set 0: the public metricsForwardPass / metricsRasterizer / metricsPass / metricsTarget)
        self.pointCloud: Optional[ops.PointCloud] = None
        self.cameraBuffer = device.createBuffer(272, "camera uniform")
        self.metricsCameraBuffer = device.createBuffer(272, "metrics camera uniform")

        self.isTraining = False
        self.iteration = 0
        self.maxIterations = 10_000
        self.stepItersPerSec = 0.0
        self.stepMs = 0.0
        self.lastDensifyPruneIteration: Optional[int] = None
        self.lastViewportWidth = self.lastViewportHeight = 1
        self.pendingPointCloudSwap: Optional[dict] = None
        self.trainCameras: list = []   # dicts: camera (float32[68]), width, height
        self.images: list = []         # dicts: texture (HipBuffer rgba8), width, height
        # held-out evaluation and the other measurements of the model: views never drawn for training and render passes of their own (evaluation.py)
        self.evaluator = evaluation.Evaluator(self)

        self.densifyPruneConfig = dict(  # trainer.ts:147-164
            schedule=dict(enabled=True, warmupIterations=500, interval=100, stopIterations=15_000),
            metricViews=10, metricDownscale=2, metricThreshold=0.5, maxBufferBytes=128 * 1024 * 1024, maxNewPointsPerStep=5000,
            pruneOpacity=0.01, cloneThresholdCount=500, splitScaleThreshold=1.0)
        self.densifyPrune = ops.DensifyPrunePass(device, self._densify_op_config())
        # batched / data-parallel step (parallel.py): fp32 gradient block, visibility counts, re-packed rows, guard word
        self._dp_grad: Optional[ops.HipBuffer] = None
        self._dp_visible: Optional[ops.HipBuffer] = None
        self._dp_rows: Optional[ops.HipBuffer] = None
        self._dp_flag: Optional[ops.HipBuffer] = None
        self._agree_word: Optional[ops.HipBuffer] = None
        # long tile lists (csrc/longlist.h): None = the library's defaults; dict(threshold=, maxItems=, maxRows=) for the passes this trainer builds
        self.longLists: Optional[dict] = None
        self._state_sliced = False  # optimizer state of non-owned slices is stale until syncOptimizerState()
        self.exchange_timing = False  # bracket the collectives with events on the device stream (bench.py)
        self._exchange_events: list = []

    DEFAULT_LANES = 3

    # ------------------------------------------------------------------ the pass sets (the reference's names are views of set 0)
    forwardPass = property(lambda self: self._train_sets[0].forwardPass if self._train_sets else None)
    rasterizer = property(lambda self: self._train_sets[0].rasterizer if self._train_sets else None)
    backwardPass = property(lambda self: self._train_sets[0].backwardPass if self._train_sets else None)
    metricsForwardPass = property(lambda self: self._metric_sets[0].forwardPass if self._metric_sets else None)
    metricsRasterizer = property(lambda self: self._metric_sets[0].rasterizer if self._metric_sets else None)
    metricsPass = property(lambda self: self._metric_sets[0].backwardPass if self._metric_sets else None)
    metricsTarget = property(lambda self: self._metric_sets[0].target if self._metric_sets else None)

    def _all_sets(self) -> list:
        """The training and metric sets: what a step and a densify event run.  (The Evaluator's sets follow the cloud and answer capacity reports on
        their own, evaluation.py.)"""
        return self._train_sets + self._metric_sets

    def _forward_passes(self) -> list:
        return [s.forwardPass for s in self._all_sets()]

    def _destroy_pass_sets(self) -> None:
        """Every pass but the optimizer's and the Evaluator's goes;``ensurePipelines`` and the first use of a metric set build them anew."""
        destroy_pass_sets(self._all_sets())
        self._train_sets, self._metric_sets = [], []

    # ------------------------------------------------------------------ configuration
    def _densify_op_config(self) -> dict:
        c = self.densifyPruneConfig
        return dict(strategy="gpu_rebuild", numViews=c["metricViews"], maxBufferBytes=c["maxBufferBytes"], maxNewPointsPerStep=c["maxNewPointsPerStep"],
                    pruneThreshold=c["pruneOpacity"], cloneThreshold=c["cloneThresholdCount"], splitThreshold=c["splitScaleThreshold"])

    def setPointCloud(self, pointCloud: ops.PointCloud) -> None:
        self.applyPointCloudSwap(dict(pointCloud=pointCloud))

    def requestPointCloudSwap(self, pointCloud: ops.PointCloud, optimizerInitialState: Optional[dict] = None) -> None:
        self.pendingPointCloudSwap = dict(pointCloud=pointCloud, optimizerInitialState=optimizerInitialState)

    def consumePointCloudSwapRequest(self) -> Optional[dict]:
        req, self.pendingPointCloudSwap = self.pendingPointCloudSwap, None
        return req

    def requestResizeTo(self, numPoints: int) -> None:
        if self.pointCloud is None:
            return
        self.requestPointCloudSwap(ops.allocatePointCloudLike(self.device, self.pointCloud, dict(numPoints=numPoints)))

    def applyPointCloudSwap(self, request: dict) -> None:
        """``trainer.ts:201-237``: adopt the new cloud (+ optimizer state) and bring the op graph to its size.  The reference destroys
        every pass and constructs new ones; here the passes are kept and resized (``setPointCloud``: buffers reused, or re-allocated
        with headroom when the cloud outgrew them) -- only the optimizer, which adopts the rebuilt state arrays, is new.  Passes that
        cannot follow (another SH degree) are rebuilt as the reference does."""
        self.drain()
        self._synchronize()
        oldParams = self.optimizer.getHyperparameters() if self.optimizer else None
        if self.optimizer is not None:
            self.optimizer.destroy()
            self.optimizer = None
        old = self.pointCloud
        self.pointCloud = request["pointCloud"]
        self._invalidate_command_buffers()
        kept = self.reuse_passes and old is not None and all(p.setPointCloud(self.pointCloud) for s in self._all_sets() for p in (s.forwardPass, s.backwardPass))
        if not kept:
            self._destroy_pass_sets()
        self.optimizer = ops.Optimizer(self.device, self.pointCloud, oldParams or self.optimizerHyperparameters, request.get("optimizerInitialState"))
        self.optimizerHyperparameters = dict(self.optimizer.getHyperparameters())
        self._dc_words = self.optimizer.setDeferredSH(self.pointCloud, True) if self.deferred_sh else None
        for fw in self._forward_passes():
            fw.setDcSource(self._dc_words)
        if old is not None and old is not self.pointCloud:
            old.gaussian_3d_buffer.destroy()
            old.sh_buffer.destroy()
        self._dp_grad = self._dp_visible = self._dp_rows = self._dp_flag = None
        self._state_sliced = False
        self.ensurePipelines(self.lastViewportWidth, self.lastViewportHeight)

    def flushPointCloud(self) -> None:
        """Brings the point cloud's SH rows up to date with what has been trained (``Optimizer.flushSH``): call before a device-side reader
        that does not go through this trainer's forward passes -- a viewer rendering the same cloud, a custom kernel.  Host reads of
        ``pointCloud.sh_buffer`` do it by themselves."""
        if self.optimizer is not None and self.pointCloud is not None:
            self.optimizer.flushSH(self.pointCloud)

    def _invalidate_command_buffers(self) -> None:
        """Recorded kernels bake pointers, viewport, hyper-parameters and loss weights: any change drops the recordings."""
        deferred = None
        if self._tickets and self.device.handle:  # steps in flight replay these recordings: wait before destroying them
            self._tickets = []
            try:
                self._synchronize()
            except ops.CapacityError as e:  # (reported once the recordings are gone: the caller must still hear of it)
                deferred = e
        for c in self._cmd_cache.values():
            c.destroy()
        self._cmd_cache = {}
        self._eager_steps = 0
        if deferred is not None:
            raise deferred

    def setDataset(self, cameras: list, images: list) -> None:
        """``cameras[i]`` pairs with ``images[i]`` (trainer.ts:575-577).  Accepted shapes: the reference's own --
        ``CameraData`` dicts from ``loaders`` and ``images.LoadedImage`` objects (the camera block is then built for the image
        size as ``Camera.set_preset`` + ``update_buffer`` do, trainer.ts:583-586) -- or ready dicts carrying ``camera`` (68
        floats) and ``width/height/texture``."""
        self.trainCameras, self.images = self._views(cameras, images)
        # one resident 272-byte camera block per training view (the reference rewrites a single uniform buffer every step)
        self._camera_buffers = [self.device.bufferFrom(np.asarray(c["camera"], np.float32)) for c in self.trainCameras]
        self._invalidate_command_buffers()

    def _views(self, cameras: list, images: list) -> tuple:
        """(camera dicts with their 68-float block, image dicts with a device texture) from the shapes ``setDataset`` accepts."""
        cameras, images = list(cameras), list(images)
        images = [im if isinstance(im, dict) else dict(name=im.name, width=im.width, height=im.height,
                                                       texture=im.texture if im.texture is not None else self.device.bufferFrom(im.bitmap))
                  for im in images]
        cameras = [c if "camera" in c else dict(c, camera=loaders.cameraUniforms(c, im["width"], im["height"])) for c, im in zip(cameras, images)]
        return cameras, images

    def getTrainingConfig(self) -> dict:
        return dict(self.trainingConfig)

    def setTrainingConfig(self, next_cfg: dict) -> None:
        """Also ``dssim_mode`` (``ops.dssim_mode``): every backward pass of the trainer, and those it builds later, differentiate that loss."""
        ops.dssim_mode(dict(self.trainingConfig, **{k: v for k, v in next_cfg.items() if v is not None}))
        self.trainingConfig.update({k: v for k, v in next_cfg.items() if v is not None})
        self._invalidate_command_buffers()
        for s in self._all_sets():
            s.backwardPass.setTrainingConfig(next_cfg)

    def getOptimizerHyperparameters(self) -> dict:
        return dict(self.optimizer.getHyperparameters() if self.optimizer else self.optimizerHyperparameters)

    def setOptimizerHyperparameters(self, next_params: dict) -> None:
        self.optimizerHyperparameters.update(next_params)
        self._invalidate_command_buffers()
        if self.optimizer:
            self.optimizer.setHyperparameters(next_params)

    def setDensifyPruneConfig(self, next_cfg: dict) -> None:
        sched = {**self.densifyPruneConfig["schedule"], **(next_cfg.get("schedule") or {})}
        self.densifyPruneConfig = {**self.densifyPruneConfig, **next_cfg, "schedule": sched}
        self.densifyPrune.setConfig(self._densify_op_config())

    def start(self) -> None:
        if self.pointCloud is None or not self.trainCameras:
            print("Cannot start training: Missing point cloud or dataset.")
            return
        self.isTraining = True
        self.iteration = 0
        self.stepItersPerSec = 0.0
        self.stepMs = 0.0
        self.lastDensifyPruneIteration = None
        # the lanes this trainer will use come into being now (the library creates a lane's stream and event at its first use, ~5 ms each:
        # otherwise the first densify event, which is the first to touch the metric lanes, pays for them -- profiles/r08t_event_timing.txt)
        for k in range(1, max(self._lanes, self.metric_lanes)):
            self.device.laneOrder(k, 0)
            self.device.laneOrder(0, k)

    def stop(self) -> None:
        self.isTraining = False
        if self.device.handle and self._tickets:
            self.drain()

    def getIsTraining(self) -> bool:
        return self.isTraining

    def setMaxIterations(self, n: int) -> None:
        self.maxIterations = max(1, int(n))

    def getMaxIterations(self) -> int:
        return self.maxIterations

    def getIteration(self) -> int:
        return self.iteration

    def getPointCount(self) -> int:
        return self.pointCloud.num_points if self.pointCloud else 0

    def getLastStepMs(self) -> float:
        return self.stepMs

    def getItersPerSec(self) -> float:
        return self.stepItersPerSec

    def getLastDensifyPruneIteration(self) -> Optional[int]:
        return self.lastDensifyPruneIteration

    def getNextDensifyPruneIteration(self) -> Optional[int]:
        s = self.densifyPruneConfig["schedule"]
        if not s["enabled"]:
            return None
        warmup, interval, stop, i = s["warmupIterations"], max(1, s["interval"]), s["stopIterations"], self.iteration
        if i >= stop:
            return None
        if i < warmup:
            return min(warmup, stop)
        nxt = warmup + math.ceil((i + 1 - warmup) / interval) * interval
        return nxt if nxt <= stop else None

    # ------------------------------------------------------------------ pipelines
    def _new_forward_pass(self, cameraBuffer, w: int, h: int, maxTileEntries: Optional[int] = None) -> ops.TiledForwardPass:
        entries = self._tile_entries() if maxTileEntries is None else int(maxTileEntries)
        fw = ops.TiledForwardPass(self.device, self.pointCloud, cameraBuffer, dict(viewportWidth=w, viewportHeight=h, renderMode="gaussian", maxTileEntries=entries))
        fw.setDcSource(self._dc_words)
        if self.longLists is not None:   # (None: the library's defaults -- threshold 2048, room for 1024 chunk slots and 8192 rows)
            fw.setLongLists(int(self.longLists.get("threshold", 2048)), int(self.longLists.get("maxItems", 0)), int(self.longLists.get("maxRows", 0)))
        return fw

    def _new_pass_set(self, cameraBuffer, w: int, h: int, *, backward: bool, max_tile_entries: Optional[int] = None) -> PassSet:
        """Forward pass, rasterizer and (``backward``) backward pass for a ``w`` x ``h`` viewport: the only place the trainer constructs them."""
        fw = self._new_forward_pass(cameraBuffer, w, h, max_tile_entries)
        rast = ops.TiledRasterizer(dict(device=self.device, forwardPass=fw, format="rgba8unorm"))
        bw = ops.TiledBackwardPass(self.device, self.pointCloud, dict(viewportWidth=w, viewportHeight=h, trainingConfig=self.trainingConfig)) if backward else None
        return PassSet(fw, rast, bw)

    def _grow_long_lists(self) -> None:
        """Long tile lists (csrc/longlist.h) work in scratch of a fixed size; a frame whose long tiles find no room is composited the ordinary way --
        correct, but as slow as its longest list.  The work's header says what the last frame wanted: looked at where the host waits anyway (a densify
        event), and every pass is given room for 1.5 x that -- up to ``longLists.maxItemsCap`` / ``maxRowsCap`` (8 192 chunk slots: 33 000 entries of
        long tiles; 65 536 rows).  A frame that wants more than the caps is FULL of long tiles (a dense cloud at a small viewport): the path is not for
        it (longlist.h: ll_frame_on) and the scratch is left alone.  (Command buffers recorded against the old scratch are dropped.)"""
        cap_items, cap_rows = int((self.longLists or {}).get("maxItemsCap", 8192)), int((self.longLists or {}).get("maxRowsCap", 65536))
        have_items = have_rows = need_items = need_rows = 0
        for fw in self._forward_passes():
            st = fw.longListStats()
            if not st["threshold"]:
                continue
            if st["stalled"]:
                warnings.warn(f"a long-list task gave up waiting (code {st['stalled']:#x}): the frame's long tiles are not to be trusted", RuntimeWarning, stacklevel=3)
            have_items, have_rows = max(have_items, st["maxItems"]), max(have_rows, st["maxRows"])
            if st["itemsWanted"] <= cap_items:
                need_items, need_rows = max(need_items, st["itemsWanted"]), max(need_rows, st["rowsWanted"])
        items = max(have_items, min(int(need_items * 1.5), cap_items)) if need_items > have_items else have_items
        rows = max(have_rows, min(int(need_rows * 1.5), cap_rows)) if need_rows > have_rows else have_rows
        if (items, rows) == (have_items, have_rows):
            return
        self.longLists = dict(self.longLists or {}, maxItems=items, maxRows=rows)
        warnings.warn(f"long-list scratch enlarged to {self.longLists['maxItems']} chunk slots and {self.longLists['maxRows']} rows", RuntimeWarning, stacklevel=3)
        self._invalidate_command_buffers()
        for fw in self._forward_passes():
            fw.setLongLists(int(self.longLists.get("threshold", 2048)), self.longLists["maxItems"], self.longLists["maxRows"])

    def ensurePipelines(self, width: int, height: int) -> None:
        if (max(1, int(width)), max(1, int(height))) != (self.lastViewportWidth, self.lastViewportHeight):
            self._invalidate_command_buffers()
        self.lastViewportWidth, self.lastViewportHeight = max(1, int(width)), max(1, int(height))
        w, h = self.lastViewportWidth, self.lastViewportHeight
        for s in self._train_sets:
            s.forwardPass.setViewport(w, h)
            s.backwardPass.setViewport(w, h)
        while len(self._train_sets) < self._op_sets:
            self._train_sets.append(self._new_pass_set(self.cameraBuffer, w, h, backward=True))
            self._gradient_output_applied = None  # (a fresh pass writes the packed gradient, the C ABI's default: _apply_gradient_output decides)
        if self.optimizer is not None and self.world_size * self.views_per_rank == 1:
            # a step whose tile-entry list overflowed is skipped on the device (and reported by the next synchronize)
            self.optimizer.setGuard(self._train_sets[0].forwardPass.getStatsBuffer(), 8)

    def ensureMetricsPipelines(self, baseWidth: int, baseHeight: int) -> tuple[int, int]:
        down = max(1, int(self.densifyPruneConfig["metricDownscale"]))
        w, h = max(1, baseWidth // down), max(1, baseHeight // down)
        if self._metric_sets and self.metricsViewportWidth == w and self.metricsViewportHeight == h:
            return w, h
        destroy_pass_sets(self._metric_sets)
        self._metric_sets = []
        self.metricsViewportWidth, self.metricsViewportHeight = w, h
        self._metric_set(0)
        return w, h

    def _metric_set(self, k: int) -> PassSet:
        """The pass set of metric lane ``k`` (``backwardPass``: its metric pass), at the metrics viewport; built on first use.  Set 0 renders through
        the trainer's ``metricsCameraBuffer``, the others through a camera block of their own."""
        w, h = self.metricsViewportWidth, self.metricsViewportHeight
        while len(self._metric_sets) <= k:
            own = len(self._metric_sets) > 0
            cam = self.device.createBuffer(272, "metrics camera uniform") if own else self.metricsCameraBuffer
            s = self._new_pass_set(cam, w, h, backward=True)
            s.target, s.cameraBuffer, s.ownsCamera = self.device.createBuffer(4 * w * h, "metrics-gt-downsampled"), cam, own
            self._metric_sets.append(s)
        return self._metric_sets[k]

    @staticmethod
    def metrics_camera(camera: np.ndarray, width: int, height: int) -> np.ndarray:
        """The metrics camera of ``trainer.ts:399-401``: ``set_preset`` keeps the view's pose and derives
        ``fovY = 2 atan(height / (2 fy))`` from the view's own height and fy (``camera.ts:196-205``), ``on_update_canvas`` turns
        it into ``focal = 0.5 canvasHeight / tan(fovY / 2)`` for the metrics canvas (``camera.ts:138-147``) and ``update_buffer``
        rebuilds projection and inverses.  The atan/tan round trip is kept: it is what the reference evaluates."""
        from . import synth
        cam = np.asarray(camera, np.float32)
        fov_y = 2.0 * math.atan(float(cam[65]) / (2.0 * float(cam[67])))
        focal = 0.5 * height / math.tan(fov_y * 0.5)
        fov_x = 2.0 * math.atan(width / (2.0 * focal))
        znear, zfar = 0.01, 100.0
        top, right = math.tan(fov_y / 2.0) * znear, math.tan(fov_x / 2.0) * znear
        out = np.zeros(68, np.float32)
        out[0:16] = cam[0:16]
        out[32], out[37] = 2.0 * znear / (2.0 * right), -2.0 * znear / (2.0 * top)   # camera.ts:29-56, column-major
        out[42], out[43], out[46] = zfar / (zfar - znear), 1.0, -(zfar * znear) / (zfar - znear)
        out[16:32] = synth.mat4_inverse(out[0:16])
        out[48:64] = synth.mat4_inverse(out[32:48])
        out[64:68] = (width, height, focal, focal)
        return out

    # ------------------------------------------------------------------ one training step
    def _encode_view(self, encoder, index: int, op_set: int = 0, geometry: bool = True, projected: bool = False) -> None:
        s = self._train_sets[op_set]
        forwardPass, rasterizer, backwardPass = s.forwardPass, s.rasterizer, s.backwardPass
        image = self.images[index]
        cam = self._camera_buffers[index]  # camera.set_preset + update_buffer (trainer.ts:583-586): the view's resident block
        forwardPass.setCameraBuffer(cam)
        if projected:   # K1 ran for all the views of the step at once (ops.projectViews): scan, emit, sort remain
            forwardPass.encodeProjected(encoder)
        else:
            forwardPass.encode(encoder)
        rasterizer.encode(encoder, image["width"], image["height"])
        res = dict(splatBuffer=forwardPass.getResources()["splatBuffer"], tileOffsetsBuffer=rasterizer.getTileOffsetsBuffer(),
                   tileIndicesBuffer=forwardPass.getSortedIndicesBuffer(), cameraBuffer=cam,
                   alphaTexture=rasterizer.getAlphaTextureView(), nContribTexture=rasterizer.getNContribTextureView())
        if geometry:
            backwardPass.encode(encoder, rasterizer.getOutputTextureView(), image["texture"], res)
        else:  # a batched step: K17 follows separately, in view order, and adds to the step's fp32 block (_step_batched)
            backwardPass.encodeRaster(encoder, rasterizer.getOutputTextureView(), image["texture"], res)

    def warmupCommandBuffers(self) -> int:
        """Records every view's command buffers up front (the first pass over a dataset does this anyway; calling it before a timed
        region keeps recording out of it).  The number of steps taken is a function of the dataset size ONLY -- never of which
        buffers this rank happens to hold already: under data parallelism every step is a collective, so all ranks must take the same
        number of them (a rank-local "skip what is recorded" here once left one rank in the exchange and its peer at the barrier).
        Two passes: the first step of a fresh trainer runs eagerly (first-use allocations), any later one records."""
        if not self.use_command_buffers or not self.isTraining or self.pointCloud is None:
            return 0
        n_views, taken = self.world_size * self.views_per_rank, 0
        for v in range(len(self.trainCameras)):
            for _ in range(2 if v == 0 else 1):
                self.step([v] * n_views)
                taken += 1
        return taken

    def step(self, view_ids: Optional[list] = None) -> None:
        """One training iteration (trainer.ts:568-660).  ``view_ids``: the global batch's views (default: drawn at random, as the
        reference picks ``Math.random()`` per step); with ``world_size > 1`` each rank takes its shard.

        Tile-entry capacity: with ``maxTileEntries`` left at 0 the forward passes size their entry lists from the cloud (30 entries per
        Gaussian, at least 2^20) -- a cloud that training has thinned out and whose survivors have grown can outrun that (c3 does, after
        ~3 000 iterations of the default schedule).  The reference truncates such a list silently; the library skips the step on the device
        and reports it.  The Trainer then doubles the lists (``_grow_tile_entry_capacity``), warns, and training goes on -- the step or two
        that were skipped are lost iterations.  A capacity the caller pinned is never touched: the error is the caller's."""
        try:
            self._step(view_ids)
        except ops.CapacityError as e:
            if not self._grow_tile_entry_capacity(e):
                raise

    def _tile_entries(self) -> int:
        """``maxTileEntries`` for a new forward pass: the caller's, or what ``_grow_tile_entry_capacity`` has arrived at (0 = the library's own sizing)."""
        return self.maxTileEntries or self._grown_tile_entries

    def _grow_tile_entry_capacity(self, error) -> bool:
        if self.maxTileEntries != 0 or not self.device.handle:
            return False
        mine, _ = ops.CapacityReports.split(error, self._own_handles())   # (a report about other owners' passes only never gets here: _settled)
        now = max([int(fw.getResources()["maxTileEntries"]) for fw in self._forward_passes()] + [self._grown_tile_entries, 1 << 20])
        new = ops.grownTileEntries(now, max([o.needed for o in mine] + [0]))
        if new <= now:
            return False
        warnings.warn(f"tile-entry lists grown from {now} to {new} entries after an overflow ({error}); the step that overflowed was skipped", RuntimeWarning, stacklevel=3)
        self._grown_tile_entries = new
        self._tickets = []
        try:
            self.device.synchronize()
        except ops.CapacityError:
            pass  # (a step still in flight overflowed as well)
        self._invalidate_command_buffers()
        # forward passes own the lists: every pass set is rebuilt around lists of the new size (as a cloud the passes cannot follow rebuilds them)
        self._destroy_pass_sets()
        self.ensurePipelines(self.lastViewportWidth, self.lastViewportHeight)
        for fw in self._forward_passes():
            fw.setDcSource(self._dc_words)
        return True

    def _step(self, view_ids: Optional[list] = None) -> None:
        if not self.isTraining or self.pointCloud is None:
            return
        stepStart = time.perf_counter()
        n_views = self.world_size * self.views_per_rank
        if view_ids is None:
            view_ids = [self._rng.randrange(len(self.trainCameras)) for _ in range(n_views)]
        mine = parallel.shard_views(view_ids, self.rank, self.world_size)
        image0 = self.images[mine[0]]
        self.ensurePipelines(image0["width"], image0["height"])

        s = self.densifyPruneConfig["schedule"]
        nextIteration = self.iteration + 1
        warmup, interval, stop = s["warmupIterations"], max(1, s["interval"]), s["stopIterations"]
        shouldDensify = s["enabled"] and warmup <= nextIteration <= stop and (nextIteration == warmup or (nextIteration - warmup) % interval == 0)

        try:
            if n_views == 1:
                self._step_single_view(mine[0])
            else:
                self._step_batched(mine)
        except BaseException as orig:
            # a failed encode (capacity, first-use allocation inside a recording, a Python error) must not leave the stream in
            # capture mode or half-recorded command buffers behind: drop the recording and fall back to a clean eager state
            if self.device.handle:
                self.device.lib.wdgs_encoder_abort(self.device.handle)
            try:
                self._invalidate_command_buffers()  # (waits for the steps still in flight before it destroys what they replay)
            except ops.CapacityError as deferred:
                # a step still in flight reported its own (deferred) overflow while the recordings were dropped: this step's error
                # stays the one raised, the deferred one rides along as its cause
                raise orig from deferred
            finally:
                self._tickets = []
            raise
        try:
            self._finish_step(n_views)
        except BaseException:
            self._tickets = []  # (the error has been consumed; whatever is still in flight is awaited by the next synchronize)
            raise

        self.iteration += 1
        self.stepMs = (time.perf_counter() - stepStart) * 1000.0
        inst = 1000.0 / self.stepMs if self.stepMs > 0 else 0.0
        self.stepItersPerSec = inst if self.stepItersPerSec == 0 else self.stepItersPerSec * 0.9 + inst * 0.1
        if shouldDensify:
            self.drain()
            self._grow_long_lists()
            self.runDensifyPruneMultiView()
            req = self.consumePointCloudSwapRequest()
            if req is not None:
                self.applyPointCloudSwap(req)
        if self.iteration >= self.maxIterations:
            self.stop()
            self.drain()

    def _run(self, key: tuple, encode) -> bool:
        """Submits the command buffer recorded under ``key``; the first time, ``encode(encoder)`` is encoded -- eagerly while the
        pipelines still allocate on first use, into a recorded command buffer (HIP graph) afterwards.  True if it was replayed."""
        cmd = self._cmd_cache.get(key)
        if cmd is not None:
            self.device.queue.submit([cmd])
            return True
        record = self.use_command_buffers and self._eager_steps >= 1
        with self.device.createCommandEncoder("trainer-" + str(key[0]), record=record) as encoder:
            encode(encoder)
            cmd = encoder.finish()
        if record:
            self._cmd_cache[key] = cmd
        self.device.queue.submit([cmd])
        return False

    def _apply_gradient_output(self) -> None:
        """The fused K17 + Adam step keeps the gradient in registers; nothing in the trainer reads the packed copy (trainer.ts hands it to
        ``optimizer.step()`` only), so the step does not write it unless asked to.  ``keep_gradients`` and ``fuse_geometry_adam`` are read
        HERE, at every step, so a host that flips them after ``setPointCloud`` is obeyed (a recorded fused step baked the old choice: the
        recordings are dropped on a change) -- ``backwardPass.getGradientsBuffer()`` never silently holds stale data."""
        want = bool(self.keep_gradients or not self.fuse_geometry_adam)
        if self._gradient_output_applied is want:
            return
        if self._gradient_output_applied is not None:
            self._invalidate_command_buffers()
        self.backwardPass.setGradientOutput(want)
        self._gradient_output_applied = want

    def _step_single_view(self, view: int) -> None:
        """The reference's step (trainer.ts:603-645): one view, Adam straight from the packed fp16 gradients."""
        self._apply_gradient_output()
        tileCounts = self._train_sets[0].forwardPass.getResources()["tileCountsBuffer"]

        def encode(encoder):
            if self.fuse_geometry_adam:  # K1..K16, then K17 + Adam + re-pack in one pass over the Gaussians
                self._encode_view(encoder, view, geometry=False)
                self.optimizer.stepWithGeometry(encoder, self.pointCloud, self.backwardPass, self._camera_buffers[view], tileCounts)
            else:
                self._encode_view(encoder, view)
                self.optimizer.step(encoder, self.pointCloud, self.backwardPass.getGradientsBuffer(), tileCounts)
        if self._run(("step", view), encode):
            self.optimizer.advanceIteration(1)
        elif not self.use_command_buffers or self._eager_steps < 1:
            self._eager_steps += 1

    def _step_batched(self, mine: list) -> None:
        """[views -> fp32 block] -> exchange -> [Adam on the owned slice] -> all-gather -> [apply the other ranks' rows].  One
        recorded command buffer per (view, op set) -- K1..K16 -- plus one each for Adam and apply, whatever the batch's composition;
        K17 is launched eagerly per view, ordered across the lanes, and adds the view's gradient to the fp32 block itself."""
        n, w = self.pointCloud.num_points, self.world_size
        sl = parallel.slice_points(n, w)
        if self._dp_grad is None:  # (allocated before any recording is opened; sized world*slice so the collectives run in place)
            self._dp_grad = self.device.createBuffer(4 * parallel.GRAD_FLOATS * w * sl, "dp-grad-f32")
            self._dp_visible = self.device.createBuffer(4 * w * sl, "dp-visible")
            self._dp_flag = self.device.createBuffer(16, "dp-guard")
            self._dp_rows = self.device.createBuffer(32 * w * sl, "dp-repacked-rows") if self._sliced else None
            self.optimizer.setGuard(self._dp_flag, 0)
        first, count = parallel.owned_range(n, w, self.rank)
        eager_before = self._eager_steps
        dev = self.device
        if self.batch_views and len(mine) <= self._op_sets:
            self._views_batched(mine)
        else:
            self._views_one_by_one(mine)
        self._timed(lambda: self.exchange.exchange_gradients(self._dp_grad.ptr, self._dp_visible.ptr, self._dp_flag.ptr, sl))
        if self._run(("adam",), lambda encoder: self.optimizer.stepF32Range(encoder, self.pointCloud, self._dp_grad, self._dp_visible, first, count, self._dp_rows)):
            self.optimizer.advanceIteration(1)
        if self._sliced:
            self._timed(lambda: self.exchange.allgather_rows(self._dp_rows.ptr, sl))
            self._run(("apply",), lambda encoder: self.optimizer.applyRepackedRows(self._dp_rows, first, count, self._dp_flag, self.pointCloud))
            self._state_sliced = w > 1
        if not self.use_command_buffers or eager_before < 1:
            self._eager_steps += 1

    def _views_batched(self, mine: list) -> None:
        """The step's views in groups (`view_group`; default: one group = all of them): [K1 of the group, one launch] -> per view, dealt to the lanes: scan, emit, sort,
        composite, loss, backward raster (one recorded command buffer per (view, place in the batch)) -> [K17 of the group, one launch,
        into the step's fp32 block, groups in view order].  The batched launches run on a lane of their own, so a group's projection and
        the previous group's K17 -- bandwidth- and latency-bound -- execute beside the other groups' rasterization kernels; each view
        waits only for its group's K1, each K17 only for its group's views."""
        dev, L = self.device, self._lanes
        sets = self._train_sets[:len(mine)]
        cams = [self._camera_buffers[v] for v in mine]
        lanes = L > 1 and self.use_command_buffers and all(("viewp", v, k) in self._cmd_cache for k, v in enumerate(mine))
        U = L if L < ops.MAX_LANES else 0          # the lane of the batched launches
        G = self.view_group or len(mine)
        groups = [list(range(g, min(g + G, len(mine)))) for g in range(0, len(mine), G)]
        try:
            if lanes:
                for s in range(1, ops.MAX_LANES if U else L):
                    dev.laneOrder(s, 0)  # every lane starts behind whatever lane 0 holds (the previous step's Adam, a densify rebuild)
            for gi, grp in enumerate(groups):   # every group's projection first, back to back on the batched launches' lane
                if lanes:
                    dev.selectLane(U)
                ops.projectViews([sets[k].forwardPass for k in grp], [cams[k] for k in grp], self.pointCloud)
                if lanes:
                    dev.laneMark(U, gi)
            for gi, grp in enumerate(groups):
                for k in grp:
                    if lanes:
                        dev.laneWaitMark(k % L, gi)  # view k starts behind its OWN group's projection
                        dev.selectLane(k % L)
                    self._run(("viewp", mine[k], k), lambda encoder, v=mine[k], k=k: self._encode_view(encoder, v, k, geometry=False, projected=True))
                    if lanes:
                        dev.laneOrder(U, k % L)      # the group's K17 follows its views (and the earlier groups' K17: lane order)
                if lanes:
                    dev.selectLane(U)
                ops.geometryViews([sets[k].backwardPass for k in grp], [cams[k] for k in grp], [sets[k].forwardPass for k in grp], self._dp_grad, self._dp_visible, self._dp_flag,
                                  self.pointCloud, continues=gi > 0)
        finally:
            if lanes:
                dev.lib.wdgs_encoder_abort(dev.handle)  # (a no-op unless an encode above failed mid-recording)
                dev.selectLane(0)
                for s in range(1, ops.MAX_LANES if U else L):
                    dev.laneOrder(0, s)  # join: the exchange and the optimizer step follow every lane

    def _views_one_by_one(self, mine: list) -> None:
        """Round 2's form: per view K1..K16 recorded, K17 eager per view, ordered across the lanes (one op set per lane)."""
        dev = self.device
        # lanes carry replays only: a step that still encodes eagerly (first-use allocations) or records keeps to lane 0
        L = min(self._lanes, self._op_sets)
        lanes = L > 1 and self.use_command_buffers and all(("view", v, k % L) in self._cmd_cache for k, v in enumerate(mine))
        try:
            for s in range(1, L if lanes else 0):
                dev.laneOrder(s, 0)  # every lane starts behind whatever lane 0 holds (the previous step's Adam, a densify rebuild)
            for k, v in enumerate(mine):
                s = k % L
                forwardPass, backwardPass = self._train_sets[s].forwardPass, self._train_sets[s].backwardPass
                if lanes:
                    dev.selectLane(s)
                self._run(("view", v, s), lambda encoder, v=v, s=s: self._encode_view(encoder, v, s, geometry=False))
                if lanes and k > 0:
                    dev.laneOrder(s, (k - 1) % L)  # the fp32 block is filled in view order: this view's sums follow the previous view's
                # K17, outside the recording (its accumulate target depends on the view's place in the batch): the first view
                # overwrites the fp32 block (no clearing pass), the others add to it; the guard word collects the views' overflow words
                backwardPass.encodeGeometry(None, self._camera_buffers[v], dict(sums=self._dp_grad, visible=self._dp_visible, first=(k == 0),
                                                                                tileCounts=forwardPass.getResources()["tileCountsBuffer"],
                                                                                guard=self._dp_flag, stats=forwardPass.getStatsBuffer()))
        finally:
            if lanes:
                dev.lib.wdgs_encoder_abort(dev.handle)  # (a no-op unless an encode above failed mid-recording)
                dev.selectLane(0)
                for s in range(1, L):
                    dev.laneOrder(0, s)  # join: the exchange and the optimizer step follow every lane

    def _timed(self, collective) -> None:
        if not self.exchange_timing:
            collective()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.device.torch_stream)
        collective()
        e1.record(self.device.torch_stream)
        self._exchange_events.append((e0, e1))

    def exchangeMilliseconds(self) -> float:
        """Device time spent between the events bracketing the collectives since ``exchange_timing`` was switched on (synchronises)."""
        self.device.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self._exchange_events)
        self._exchange_events = []
        return float(ms)

    def _metric_overflow(self):
        """The capacity report of this rank's metric forward passes (their sticky words are consumed), or None.  Synchronises."""
        found = None
        for s in self._metric_sets:
            try:
                s.forwardPass.check()
            except ops.CapacityError as e:
                found = found or e
        return found

    def _agree(self, flag: bool) -> bool:
        """True on every rank if ``flag`` is true on any: one u32 summed over the ranks on the device, read back (a host wait -- only used inside a
        densify event, which reads the rebuilt cloud's size back anyway)."""
        if self.world_size <= 1:
            return bool(flag)
        if self._agree_word is None:
            self._agree_word = self.device.createBuffer(4, "agreement word")
        self._agree_word.write(np.array([1 if flag else 0], np.uint32))
        self.exchange.allreduce_counts(self._agree_word.ptr, 1)
        return int(self._agree_word.read(np.uint32, 1)[0]) != 0

    def _own_handles(self) -> list:
        return [int(fw.handle.value or 0) for fw in self._forward_passes()]

    def _settled(self, wait) -> None:
        """``wait()`` with the capacity reports sorted by owner (``ops.CapacityReports.settle``).  A report with a line about THIS trainer's passes is
        raised -- also one that another owner's wait consumed and left for us (a Viewer reading its frame).  Lines about passes this trainer does not
        own -- a Viewer rendering the same cloud on this device: the report is device-wide, whoever waits first gets it -- are left for the passes'
        owner, who has to enlarge its lists; the trainer says so once."""
        s = self.device.capacityReports.settle(self._own_handles(), wait)
        if s.foreign and not self._foreign_overflow_warned:
            left = self.device.capacityReports.pending[-1]   # (what settle has just posted)
            warnings.warn(f"a forward pass that is not this trainer's overflowed its tile-entry lists ({left}); its owner has to enlarge them", RuntimeWarning, stacklevel=4)
            self._foreign_overflow_warned = True
        if s.mine:
            raise s.error

    def _wait(self, ticket) -> None:
        self._settled(lambda: self.device.queue.wait(ticket))

    def _synchronize(self) -> None:
        self._settled(self.device.synchronize)

    def _finish_step(self, n_views: int) -> None:
        """``await onSubmittedWorkDone()`` (trainer.ts:639-645) + the deferred capacity check, for the step ``pipeline_depth - 1``
        submissions ago.  In a batched step the guard word was summed over all ranks by the exchange and the optimizer kernels leave
        a host-visible note when they skip themselves, so every rank raises at the same step."""
        self._tickets.append(self.device.queue.mark())
        while len(self._tickets) >= self.pipeline_depth:
            self._wait(self._tickets.pop(0))

    def drain(self) -> None:
        """Awaits every step still in flight (a no-op at ``pipeline_depth`` 1)."""
        tickets, self._tickets = self._tickets, []
        for t in tickets:
            self._wait(t)

    def syncOptimizerState(self) -> None:
        """Brings every rank's optimizer state up to date: after sliced steps a rank holds current (param, m, v) only for the
        Gaussians it owns; each owner broadcasts its slice of the six state arrays.  A no-op on one rank.  Called before a
        densify rebuild; call it before reading ``optimizer.getStateBuffers()`` in a multi-rank run."""
        if not self._state_sliced or self.world_size <= 1:
            return
        n, w = self.pointCloud.num_points, self.world_size
        bufs = self.optimizer.getStateBuffers()  # flushes the compact SH-DC copy into paramSH / stateSH first
        rows = dict(optPosBuffer=48, optRotBuffer=48, optScaleBuffer=48, optOpacityBuffer=12, paramSH=192, stateSH=384)
        for root in range(w):
            first, count = parallel.owned_range(n, w, root)
            for k, rb in rows.items():
                self.exchange.broadcast(bufs[k].ptr + first * rb, count * rb, root)
        self.optimizer.stateChanged()
        self._state_sliced = False

    def destroy(self) -> None:
        """Deterministic teardown: command buffers, then every op, then the buffers this trainer allocated.  The device itself
        belongs to the caller (``HipDevice.destroy()`` comes after this, and before ``torch.distributed.destroy_process_group``)."""
        if self.device.handle:
            self.device.lib.wdgs_encoder_abort(self.device.handle)
            self._tickets = []
            try:
                self.device.synchronize()
            except ops.CapacityError:
                pass  # (a deferred report about a step of a trainer that is going away)
        self._invalidate_command_buffers()
        self._destroy_pass_sets()
        self.evaluator.destroy()
        for op in (self.optimizer, self.densifyPrune):
            if op is not None:
                op.destroy()
        self.optimizer = self.densifyPrune = None
        self._dp_grad = self._dp_visible = self._dp_rows = self._dp_flag = None
        self._camera_buffers = []
        self.pointCloud = None
        self.isTraining = False

    # ------------------------------------------------------------------ evaluation and analysis: all of it is the Evaluator's (evaluation.py)
    evalCameras = property(lambda self: self.evaluator.cameras)
    evalImages = property(lambda self: self.evaluator.images)
    evalMaxTileEntries = property(lambda self: self.evaluator.maxTileEntries, lambda self, n: setattr(self.evaluator, "maxTileEntries", n),
                                  doc="tile-entry lists of the Evaluator's passes (0: what the training passes get)")

    def setEvaluationViews(self, cameras: list, images: list) -> None:
        """``Evaluator.setEvaluationViews``: views to evaluate on and never to train on."""
        self.evaluator.setEvaluationViews(cameras, images)

    def evaluate(self, viewIds: Optional[list] = None, split: str = "eval") -> dict:
        """``Evaluator.evaluate``: PSNR and SSIM of the current model on the evaluation or the training views; training is untouched."""
        return self.evaluator.evaluate(viewIds, split)

    def normalConsistency(self, viewIds: Optional[list] = None, split: str = "eval", depthKind: str = "median") -> dict:
        """``Evaluator.normalConsistency``: agreement of the composited normals with the normals of the model's own depth map."""
        return self.evaluator.normalConsistency(viewIds, split, depthKind)

    def meshDepthAgreement(self, mesh: dict, viewIds: Optional[list] = None, split: str = "eval", depthKind: str = "median", **options) -> dict:
        """``Evaluator.meshDepthAgreement``: a mesh rasterized under each view against the model's own depth map of that view."""
        return self.evaluator.meshDepthAgreement(mesh, viewIds, split, depthKind, **options)

    def meshVisibility(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median", **options) -> dict:
        """``Evaluator.meshVisibility``: per face of a mesh the pixels and views that show it, and the pixels where the model's depth agrees."""
        return self.evaluator.meshVisibility(mesh, viewIds, split, depthKind, **options)

    def cullMesh(self, mesh: dict, minPixels: int = 1, minViews: int = 1, minAgreeing: int = 0, minAgreeingFraction: float = 0.0, **visibilityOptions) -> dict:
        """``Evaluator.cullMesh``: a mesh without the faces the views do not see (``meshVisibility``, ``ops.selectFaces``' rule and ``ops.filterFaces``,
        flags and compaction on the device)."""
        return self.evaluator.cullMesh(mesh, minPixels, minViews, minAgreeing, minAgreeingFraction, **visibilityOptions)

    def bakeMeshColours(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", **options) -> dict:
        """``Evaluator.bakeMeshColours``: a mesh with its vertex colours taken from the split's photographs under the split's cameras."""
        return self.evaluator.bakeMeshColours(mesh, viewIds, split, **options)

    def bakeMeshTexture(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", **options) -> dict:
        """``Evaluator.bakeMeshTexture``: a mesh with a texture atlas taken from the split's photographs under the split's cameras."""
        return self.evaluator.bakeMeshTexture(mesh, viewIds, split, **options)

    def fuseDepth(self, volume: ops.TSDFVolume, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median") -> list:
        """``Evaluator.fuseDepth``: fuses the current model's depth maps into ``volume``."""
        return self.evaluator.fuseDepth(volume, viewIds, split, depthKind)

    def extractMesh(self, lo, hi, voxelSize: float, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median", minWeight: float = 1.0,
                    keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0, weld: str = "host", simplify: Optional[float] = None,
                    smooth: Optional[int] = None, normals: bool = False, cull: Optional[dict] = None, bake=None, texture=None, **volumeOptions) -> dict:
        """``Evaluator.extractMesh``: the current model as a triangle mesh of the box ``[lo, hi]``, welded on the host or (``weld="device"``) on the device;
        with ``cull=dict(...)`` without the faces no view sees (``cullMesh``'s rule and options), with ``smooth=iterations`` Taubin-smoothed, with
        ``simplify=cellSize`` then simplified by vertex clustering, with ``normals=True`` given the final mesh's vertex normals, with ``bake=True`` or
        ``bake=dict(...)`` coloured from the photographs (``bakeMeshColours``' options), with ``texture=True`` or ``texture=dict(...)`` given a texture
        atlas from them (``bakeMeshTexture``'s options)."""
        return self.evaluator.extractMesh(lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld=weld,
                                          simplify=simplify, smooth=smooth, normals=normals, cull=cull, bake=bake, texture=texture, **volumeOptions)

    def evaluateGeometry(self, reference, lo, hi, voxelSize: float, maxDistance: float, threshold: float, density: Optional[float] = None, seed: int = 0,
                         keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0, **extractMeshOptions) -> dict:
        """``Evaluator.evaluateGeometry``: the extracted mesh scored against a reference point set."""
        return self.evaluator.evaluateGeometry(reference, lo, hi, voxelSize, maxDistance, threshold, density, seed, keepLargest, minTriangles, minFraction,
                                               **extractMeshOptions)

    def contributionStats(self, viewIds: Optional[list] = None, split: str = "train") -> dict:
        """``Evaluator.contributionStats``: how much of each Gaussian the views' images hold."""
        return self.evaluator.contributionStats(viewIds, split)

    # ------------------------------------------------------------------ contribution-based pruning (no reference counterpart)
    def pruneByContribution(self, minMaxWeight: float = 0.0, minWeightSum: float = 0.0, minPixels: int = 0, fraction: float = 0.0,
                            viewIds: Optional[list] = None) -> dict:
        """Removes the Gaussians the training views (``viewIds``: all) need least: a Gaussian is kept iff it meets every criterion given --
        its largest weight ``>= minMaxWeight``, its weight sum ``>= minWeightSum``, its pixel count ``>= minPixels``, and, with ``fraction`` f,
        its ``sum_q`` not below the k-th smallest ``sum_q`` of the cloud, k = floor(f N) (at most k go; ties at the boundary stay).  The
        survivors, their SH rows and their optimizer state are compacted in index order, bit for bit, and the cloud is swapped as after a densify
        event (optimizer iteration and state handed over).  ``dict(before, after, pruned)``; pruning nothing or everything (a warning) leaves the
        cloud as it is.  Single rank only."""
        if self.world_size > 1:
            raise RuntimeError("pruneByContribution: world_size > 1 is not supported (the replicas would have to agree on the statistics)")
        if not (minMaxWeight >= 0 and minWeightSum >= 0 and minPixels >= 0 and 0 <= fraction < 1):
            raise ValueError("pruneByContribution: the thresholds must be >= 0 and fraction in [0, 1)")
        if not (minMaxWeight or minWeightSum or minPixels or fraction):
            raise ValueError("pruneByContribution: give at least one of minMaxWeight, minWeightSum, minPixels, fraction")
        if self.optimizer is None or self.densifyPrune is None:
            raise RuntimeError("pruneByContribution: no point cloud")
        stats, _ = self.evaluator.contributionBuffer(viewIds, "train", "pruneByContribution")
        try:
            n = self.pointCloud.num_points
            unchanged = dict(before=n, after=n, pruned=0)
            rule = dict(minMaxWeight=float(minMaxWeight), minWeightSum=float(minWeightSum), minPixels=int(minPixels), minSumQ=0)
            k = int(math.floor(fraction * n))
            if k > 0:
                rule["minSumQ"] = int(np.partition(ops.readContribution(stats, n)["sum_q"], k - 1)[k - 1])
            if not any(rule.values()):
                return unchanged   # (only a fraction was given, and it selects nothing: k = 0, or the k-th smallest sum is 0)
            dp = self.densifyPrune
            dp.ensureSize(n)
            dp.encodeContributionDecision(None, n, stats, rule)
            offsets = dp.encodePrefixSum(None)
            dp.encodeTotalOut(None)
            outN = dp.readTotal()
            if outN == n:
                return unchanged
            if outN == 0:
                warnings.warn("pruneByContribution: the criteria would remove every Gaussian; the cloud is left as it is", RuntimeWarning, stacklevel=2)
                return unchanged
            self.optimizer.flushSH(self.pointCloud)  # the rebuild copies the cloud's SH rows: bring the deferred DC halves in first
            outPointCloud = ops.allocatePointCloudLike(self.device, self.pointCloud, dict(numPoints=outN))
            outState = ops.allocateOptimizerStateBuffers(self.device, outN)
            dp.encodeScatter(None, dict(pointCloud=self.pointCloud, optimizerState=self.optimizer.getStateBuffers(), outOffsetBuffer=offsets, outNumPoints=outN,
                                        resetNewOptimizerState=False), dict(outPointCloud=outPointCloud, outOptimizerState=outState))
            self._synchronize()
            self.applyPointCloudSwap(dict(pointCloud=outPointCloud, optimizerInitialState=dict(iteration=self.optimizer.getIteration(), buffers=outState)))
            return dict(before=n, after=outN, pruned=n - outN)
        finally:
            stats.destroy()

    # ------------------------------------------------------------------ densify / prune
    def runDensifyPruneMultiView(self) -> None:
        if self.pointCloud is None or self.optimizer is None or not self.trainCameras or not self.images:
            return
        baseW, baseH = self.lastViewportWidth, self.lastViewportHeight
        mW, mH = self.ensureMetricsPipelines(baseW, baseH)
        c = self.densifyPruneConfig
        viewsTarget = max(1, int(c["metricViews"]))
        encoder = self.device.createCommandEncoder("densify-prune multiview metrics")
        counts = self.metricsPass.getMetricCountsBuffer()
        encoder.clearBuffer(counts)
        dev, L = self.device, self.metric_lanes
        usedViews, attempts, taken = 0, 0, 0
        try:
            while attempts < viewsTarget * 4 and usedViews < viewsTarget:
                attempts += 1
                idx = self._rng.randrange(len(self.trainCameras))
                camData, image = self.trainCameras[idx], self.images[idx]
                if image["width"] != baseW or image["height"] != baseH:
                    continue
                # every rank walks the same view list; the work is sharded round-robin and the counts are all-reduced below
                take = (usedViews % self.world_size) == self.rank
                usedViews += 1
                if not take:
                    continue
                k = taken % L   # this rank's views in turn on its metric lanes; every lane's pass adds into set 0's counts
                taken += 1
                s = self._metric_set(k)
                fw, rast, mpass, target, cam = s.forwardPass, s.rasterizer, s.backwardPass, s.target, s.cameraBuffer
                if k > 0:
                    if taken <= L:   # the lane's first view of this event: behind the clear (and whatever else lane 0 holds)
                        mpass.setMetricCountsTarget(counts)
                        dev.laneOrder(k, 0)
                    dev.selectLane(k)
                cam.write(self.metrics_camera(camData["camera"], mW, mH))
                fw.encode(encoder)
                rast.encode(encoder, mW, mH)
                ops.downsampleRGBA8(dev, image["texture"], baseW, baseH, target, mW, mH)
                mpass.computeMetricMap(encoder, rast.getOutputTextureView(), target, dict(threshold=c["metricThreshold"]))
                mpass.computeMetricCounts(encoder, dict(splatBuffer=fw.getResources()["splatBuffer"], tileOffsetsBuffer=rast.getTileOffsetsBuffer(),
                                                       tileIndicesBuffer=fw.getSortedIndicesBuffer(), nContribTexture=rast.getNContribTextureView()), dict(clear=False))
                if k > 0:
                    dev.selectLane(0)
        finally:
            dev.selectLane(0)
            for k in range(1, min(L, taken)):
                dev.laneOrder(0, k)   # join: normalize / prepare / the exchange follow every lane
        if usedViews == 0:
            return
        if self.world_size > 1:
            # A metric pass whose tile-entry list overflowed has counted a truncated view: the event is void -- and it has to be void on EVERY rank
            # (the views are sharded, so one rank alone may overflow; were it to bail out while its peers rebuild the cloud, the replicas
            # would part and the next exchange hang).  Each rank looks at its own metric passes, the flags are summed over the ranks, and all skip the
            # event together, before any count has been exchanged; a rank that overflowed raises on the way out, which makes step() enlarge its lists.
            overflow = self._metric_overflow()
            if self._agree(overflow is not None):
                if overflow is not None:
                    raise overflow
                return
            # u32 sum on the device, in place in the pass's own buffer (SURVEY 8(e) "Determinism")
            self.exchange.allreduce_counts(self.metricsPass.getMetricCountsBuffer().ptr, self.pointCloud.num_points)
        self.metricsPass.normalizeMetricCounts(encoder, dict(divisor=usedViews))
        self.densifyPrune.ensureSize(self.pointCloud.num_points)
        prepared = self.densifyPrune.encodePrepare(encoder, dict(pointCloud=self.pointCloud, metricCountsBuffer=self.metricsPass.getMetricCountsBuffer()))
        outTotal = self.densifyPrune.readTotal()  # the one 4-byte read-back (trainer.ts:440-458)
        inN = self.pointCloud.num_points
        outN = min(outTotal, prepared["maxOutPoints"])
        if outN == 0 or outN == inN:
            return
        self.syncOptimizerState()  # every rank rebuilds the whole cloud, so every rank needs the whole state
        self.optimizer.flushSH(self.pointCloud)  # the rebuild copies the cloud's SH rows: bring the deferred DC halves in first
        outPointCloud = ops.allocatePointCloudLike(self.device, self.pointCloud, dict(numPoints=outN))
        outState = ops.allocateOptimizerStateBuffers(self.device, outN)
        self.densifyPrune.encodeScatter(encoder, dict(pointCloud=self.pointCloud, optimizerState=self.optimizer.getStateBuffers(),
                                                      outOffsetBuffer=prepared["outOffsetBuffer"], outNumPoints=outN, resetNewOptimizerState=True),
                                        dict(outPointCloud=outPointCloud, outOptimizerState=outState))
        self._synchronize()
        self.requestPointCloudSwap(outPointCloud, dict(iteration=self.optimizer.getIteration(), buffers=outState))
        self.lastDensifyPruneIteration = self.iteration
