"""``Evaluator`` -- everything a ``Trainer`` can measure about its model without training it: held-out evaluation, normal consistency, TSDF fusion
and mesh extraction, geometry metrics, render contribution.  None of it has a counterpart in the reference.

It renders through pass sets of its own (no backward pass), one per image size, built on first use and following the trainer's cloud, and answers
the capacity reports about them itself (``ops.CapacityReports.settle``).  ``Trainer`` keeps the public methods and delegates to its Evaluator; what
"training is untouched" rests on is the short list of trainer members in the class docstring below.
"""
from __future__ import annotations

import time
import warnings
from typing import Optional

import numpy as np

from . import loaders, ops
from .trainer import PassSet, destroy_pass_sets


class Evaluator:
    """The evaluation side of one ``Trainer``.  It owns the evaluation views with their camera blocks, the per-size evaluation ``PassSet``s, the size
    an overflow has grown their tile-entry lists to and the long-list settings they were built with.

    The seam -- the only members of the trainer used here:
      * ``device``, ``pointCloud``, ``iteration``;
      * ``trainCameras``, ``images``, ``_camera_buffers``: the training views, for ``split="train"``;
      * ``_views``: the camera and image shapes ``setDataset`` accepts;
      * ``_new_pass_set``: carries the live SH-DC words and the trainer's long-list settings;  ``_dc_words``, ``longLists``;
      * ``drain()`` and ``_grow_tile_entry_capacity()``: a training step still in flight is awaited, its overflow answered as ``step()`` would.
    Never the training or metric pass sets, the command-buffer cache, the tickets, the RNG, the optimizer or the densify pass."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.device = trainer.device
        self.cameras: list = []
        self.images: list = []
        self._camera_buffers: list = []
        self._sets: dict = {}
        self.maxTileEntries = 0       # tile-entry lists of the evaluation passes (0: what the training passes get)
        self._tile_entries = 0        # (what an overflowing evaluation view has made of them)
        self._long_lists: Optional[dict] = None

    def destroy(self) -> None:
        self._destroy_sets()
        self._camera_buffers = []

    # ------------------------------------------------------------------ views and pass sets
    def setEvaluationViews(self, cameras: list, images: list) -> None:
        """Views to evaluate on and never to train on (``loaders.holdoutSplit`` gives the every-8th test views of the 3DGS convention).  Same
        shapes as ``setDataset``; the images may have another size than the training images."""
        cameras, images = list(cameras), list(images)
        if len(cameras) != len(images):
            raise ValueError(f"setEvaluationViews: {len(cameras)} cameras, {len(images)} images")
        self.cameras, self.images = self.trainer._views(cameras, images)
        self._camera_buffers = [self.device.bufferFrom(np.asarray(c["camera"], np.float32)) for c in self.cameras]

    def _destroy_sets(self) -> None:
        destroy_pass_sets(self._sets.values())
        self._sets = {}

    def _set(self, width: int, height: int, cameraBuffer) -> PassSet:
        """The pass set (no backward pass) for one image size: built through the trainer's ``_new_pass_set`` (the live SH-DC words, its long-list
        settings), with lists of ``_tile_entries`` if an evaluation view has outgrown the training passes' size.  Never a guard."""
        key = (int(width), int(height))
        if key not in self._sets:
            self._sets[key] = self.trainer._new_pass_set(cameraBuffer, key[0], key[1], backward=False, max_tile_entries=self._tile_entries or self.maxTileEntries or None)
        return self._sets[key]

    def _follow_cloud(self) -> None:
        """Brings the passes to the trainer's current cloud (a swap after a densify event, another size) and its current long-list settings."""
        t = self.trainer
        if self._long_lists != t.longLists:
            self._destroy_sets()
            self._long_lists = None if t.longLists is None else dict(t.longLists)
        for s in list(self._sets.values()):
            if s.forwardPass.pointCloud is not t.pointCloud and not s.forwardPass.setPointCloud(t.pointCloud):
                self._destroy_sets()   # (another SH degree: built anew below)
                break
        for s in self._sets.values():
            s.forwardPass.setDcSource(t._dc_words)

    def _overflow(self) -> Optional[int]:
        """Waits for the evaluation renders; the entries the largest overflowing one needed, or None (other owners' lines are left for them)."""
        mine = self.device.capacityReports.settle((int(s.forwardPass.handle.value or 0) for s in self._sets.values()), self.device.synchronize).mine
        return max(o.needed for o in mine) if mine else None

    def _views(self, what: str, viewIds: Optional[list], split: str) -> tuple:
        """(cameras, images, camera buffers, view ids) of a split, checked: what ``evaluate``, ``normalConsistency`` and ``contributionStats`` start with."""
        t = self.trainer
        if split not in ("eval", "train"):
            raise ValueError(f"{what}: split must be 'eval' or 'train', not {split!r}")
        if t.pointCloud is None:
            raise RuntimeError(f"{what}: no point cloud")
        cams, imgs, bufs = ((self.cameras, self.images, self._camera_buffers) if split == "eval" else
                            (t.trainCameras, t.images, t._camera_buffers))
        ids = list(range(len(cams))) if viewIds is None else [int(v) for v in viewIds]
        for v in ids:
            if not 0 <= v < len(cams):
                raise IndexError(f"{what}: view {v} of {len(cams)} ({split})")
        return cams, imgs, bufs, ids

    def _drain(self) -> None:
        """Drains the trainer's pipeline in front of renders through the evaluation passes."""
        try:
            self.trainer.drain()
        except ops.CapacityError as e:   # a training step's overflow, as step() would have met it at its next wait
            if not self.trainer._grow_tile_entry_capacity(e):
                raise

    def _render_views(self, ids: list, imgs: list, bufs: list, each, restart=None, what: str = "evaluate") -> None:
        """The render loop: every view of ``ids`` through the evaluation pass set of its size, then ``each(i, v, passSet, width, height)``; after
        an overflow the lists are grown, ``restart()`` is called and ALL views are rendered again."""
        while ids:
            self._follow_cloud()
            for i, v in enumerate(ids):
                w, h = int(imgs[v]["width"]), int(imgs[v]["height"])
                s = self._set(w, h, bufs[v])
                fw, rast = s.forwardPass, s.rasterizer
                fw.setCameraBuffer(bufs[v])
                fw.encode(None)
                rast.encode(None, w, h)
                each(i, v, s, w, h)
            needed = self._overflow()
            if needed is None:
                break
            now = max([int(s.forwardPass.getResources()["maxTileEntries"]) for s in self._sets.values()] + [self._tile_entries])
            new = ops.grownTileEntries(now, needed)
            if new <= now:
                raise RuntimeError(f"{what}: a view needs {needed} tile entries, more than the lists can hold")
            warnings.warn(f"evaluation tile-entry lists grown from {now} to {new} entries after an overflow; the views are rendered again", RuntimeWarning, stacklevel=4)
            self._tile_entries = new
            self._destroy_sets()
            if restart is not None:
                restart()

    # ------------------------------------------------------------------ held-out evaluation
    def evaluate(self, viewIds: Optional[list] = None, split: str = "eval") -> dict:
        """PSNR and SSIM of the current model on the evaluation views (``split="eval"``, ``setEvaluationViews``) or on training views
        (``split="train"``): ``dict(iteration, views, psnr=[...], ssim=[...], mean_psnr, mean_ssim, ms)``.  PSNR comes from the exact SSE kernel
        (``inf`` for identical images); SSIM is ``ops.imageSSIM``'s; the means are means of the per-view values; ``ms`` the call's wall time.

        Drains the pipeline, then renders every view through passes of its own and writes view i's SSE and SSIM into slot i of two device arrays,
        read back once at the end.  A view whose tile-entry list overflowed is rendered again with larger lists -- never reported from a truncated
        render.  Training is untouched: no RNG draw, no training pass, no recording dropped; a trainer that evaluates every few steps follows the
        same trajectory as one that never does.  Per rank with ``world_size > 1`` (no collective)."""
        cams, imgs, bufs, ids = self._views("evaluate", viewIds, split)
        t0 = time.perf_counter()
        self._drain()
        n = len(ids)
        out = self.device.createBuffer(16 * max(1, n), "evaluation sse + ssim")
        sse_at, ssim_at = out.ptr, out.ptr + 8 * max(1, n)
        try:
            def measure(i, v, s, w, h):
                pred = s.rasterizer.getOutputTextureView()
                ops.encodeImageSSE(self.device, pred, imgs[v]["texture"], w * h, self.device.view(sse_at + 8 * i, 8))
                ops.encodeImageSSIM(self.device, pred, imgs[v]["texture"], w, h, self.device.view(ssim_at + 8 * i, 8))
            self._render_views(ids, imgs, bufs, measure, what="evaluate")
            sse = out.read(np.uint64, count=n) if n else np.zeros(0, np.uint64)
            ssim = out.read(np.float64, count=n, offset=8 * max(1, n)) if n else np.zeros(0)
        finally:
            out.destroy()
        psnr = [ops.psnrFromSSE(int(sse[i]), int(imgs[v]["width"]) * int(imgs[v]["height"])) for i, v in enumerate(ids)]
        ssim_l = [float(x) for x in ssim]
        return dict(iteration=self.trainer.iteration, views=ids, psnr=psnr, ssim=ssim_l, sse=[int(x) for x in sse],
                    mean_psnr=float(np.mean(psnr)) if n else float("nan"), mean_ssim=float(np.mean(ssim_l)) if n else float("nan"),
                    ms=(time.perf_counter() - t0) * 1e3)

    # ------------------------------------------------------------------ normal consistency
    def normalConsistency(self, viewIds: Optional[list] = None, split: str = "eval", depthKind: str = "median") -> dict:
        """How well the composited normals of the current model agree with the normals of its own depth map, per view: a geometry score that needs no
        ground truth (a surface scores near 0, a fog near 1).  ``dict(iteration, views, value=[...], pixels=[...], sum_e=[...], sum_a=[...], mean, ms)``:
        ``value`` is ``ops.normalAgreement``'s weight-averaged ``1 - cos`` between ``encodeNormal``'s image and ``ops.depthToNormals`` of the
        ``depthKind`` depth image (nan for a view where no pixel counts), ``mean`` the same average over all views' pixels (``sum sum_e / sum sum_a``).

        Rendered through evaluate's passes, with its isolation: the pipeline is drained, a view whose lists overflowed is rendered again, no RNG draw,
        no training pass, no recording dropped; ``evaluate()``'s result is what it was.  Per rank with ``world_size > 1``."""
        if depthKind not in ("median", "expected"):
            raise ValueError(f"normalConsistency: depthKind must be 'median' or 'expected', not {depthKind!r}")
        cams, imgs, bufs, ids = self._views("normalConsistency", viewIds, split)
        t0 = time.perf_counter()
        self._drain()
        n = len(ids)
        out = self.device.createBuffer(24 * max(1, n), "normal agreement sums")
        scratch = self.device.createBuffer(16 * max([1] + [int(imgs[v]["width"]) * int(imgs[v]["height"]) for v in ids]), "depth normals")
        try:
            def measure(i, v, s, w, h):
                s.rasterizer.encodeDepth(None, (depthKind,))
                s.rasterizer.encodeNormal(None)
                ops.depthToNormals(self.device, s.rasterizer.getDepthTextureView(depthKind), w, h, cams[v]["camera"], scratch)
                ops.encodeNormalAgreement(self.device, s.rasterizer.getNormalTextureView(), scratch, w, h, self.device.view(out.ptr + 24 * i, 24))
            self._render_views(ids, imgs, bufs, measure, what="normalConsistency")
            sums = (out.read(np.uint64, count=3 * n) if n else np.zeros(0, np.uint64)).reshape(n, 3)
        finally:
            scratch.destroy()
            out.destroy()
        sum_e, sum_a, pixels = ([int(x) for x in sums[:, k]] for k in range(3))
        return dict(iteration=self.trainer.iteration, views=ids, value=[(e / a) if a else float("nan") for e, a in zip(sum_e, sum_a)], pixels=pixels,
                    sum_e=sum_e, sum_a=sum_a, mean=(sum(sum_e) / sum(sum_a)) if sum(sum_a) else float("nan"), ms=(time.perf_counter() - t0) * 1e3)

    # ------------------------------------------------------------------ a mesh against the model's own depth maps
    def meshDepthAgreement(self, mesh: dict, viewIds: Optional[list] = None, split: str = "eval", depthKind: str = "median", maxDifference: float = 1.0,
                           threshold: float = 0.05, minWeightSum: float = 0.5, near: float = ops.MESH_RASTER_NEAR, cull: str = "none") -> dict:
        """How far ``mesh`` (``ops.rasterizeMesh``'s: numpy or a dict of ``HipBuffer``) agrees with the model it came from, view by view, with no reference
        geometry: per view the model's ``depthKind`` depth map (``b``; present where its weight sum is at least ``minWeightSum``) against the mesh
        rasterized under the same camera (``a``), through ``ops.encodeDepthAgreement``.  ``dict(iteration, views, both=[...], onlyA=[...], onlyB=[...],
        within=[...], sum_q=[...], mean=[...], total=dict(both, onlyA, onlyB, within, sum_q, mean), ms)``: ``onlyB`` pixels are where the model sees
        surface and the mesh has a hole, ``onlyA`` where the mesh has surface the model does not show; ``mean`` is the mean absolute depth difference
        over ``both``, clamped at ``maxDifference``; ``within`` counts differences of at most ``threshold``.

        Rendered through evaluate's passes, with its isolation: the pipeline is drained, a view whose lists overflowed is rendered again, no RNG draw,
        no training pass, no recording dropped.  Per rank with ``world_size > 1``."""
        if depthKind not in ("median", "expected"):
            raise ValueError(f"meshDepthAgreement: depthKind must be 'median' or 'expected', not {depthKind!r}")
        cams, imgs, bufs, ids = self._views("meshDepthAgreement", viewIds, split)
        t0 = time.perf_counter()
        self._drain()
        n = len(ids)
        dev = self.device
        vertices, faces, V, F, own = ops._mesh_on_device(dev, mesh, "meshDepthAgreement")
        out = dev.createBuffer(40 * max(1, n), "depth agreement sums")
        sizes = [(int(imgs[v]["width"]), int(imgs[v]["height"])) for v in ids]
        scratch = dev.createBuffer(4 * max([1] + [w * h for w, h in sizes]), "mesh depth")
        rasterizer = ops.MeshRasterizer(dev)
        try:
            if sizes:   # (grown once, to the largest view, in front of the loop)
                w, h = max(sizes, key=lambda s: s[0] * s[1])
                rasterizer.encode(vertices, V, faces, F, None, bufs[ids[0]], w, h, near, cull, depth=scratch)

            def measure(i, v, s, w, h):
                s.rasterizer.encodeDepth(None, (depthKind, "weight_sum"))
                rasterizer.encode(vertices, V, faces, F, None, bufs[v], w, h, near, cull, depth=scratch)
                ops.encodeDepthAgreement(dev, scratch, s.rasterizer.getDepthTextureView(depthKind), w, h, maxDifference, threshold, dev.view(out.ptr + 40 * i, 40),
                                         bWeightSum=s.rasterizer.getDepthTextureView("weight_sum"), minWeightSum=minWeightSum)
            self._render_views(ids, imgs, bufs, measure, what="meshDepthAgreement")
            sums = (out.read(np.uint64, count=5 * n) if n else np.zeros(0, np.uint64)).reshape(n, 5)
        finally:
            rasterizer.destroy()
            scratch.destroy()
            out.destroy()
            if own:
                vertices.destroy()
                faces.destroy()
        per = [ops._depth_agreement_result(row, maxDifference) for row in sums]
        result = dict(iteration=self.trainer.iteration, views=ids)
        for k in ("both", "onlyA", "onlyB", "within", "sum_q", "mean"):
            result[k] = [p[k] for p in per]
        result["total"] = ops._depth_agreement_result([sum(int(row[k]) for row in sums) for k in range(5)], maxDifference)
        result["ms"] = (time.perf_counter() - t0) * 1e3
        return result

    # ------------------------------------------------------------------ which faces of a mesh the views see
    def _face_visibility(self, what: str, vertices, faces, V: int, F: int, viewIds, split: str, depthKind: str, threshold: float, minWeightSum: float, near: float,
                         cull: str) -> tuple:
        """``(visibility, view ids, totals)``: an ``ops.FaceVisibility`` of the mesh on the device accumulated over the views -- the caller destroys it --
        and its cumulative totals after each view.  ``meshDepthAgreement``'s loop: the rasterizer grown once, one encode and one accumulate per view."""
        if depthKind not in ("median", "expected"):
            raise ValueError(f"{what}: depthKind must be 'median' or 'expected', not {depthKind!r}")
        cams, imgs, bufs, ids = self._views(what, viewIds, split)
        self._drain()
        dev = self.device
        sizes = [(int(imgs[v]["width"]), int(imgs[v]["height"])) for v in ids]
        npix = max([1] + [w * h for w, h in sizes])
        depth, image = dev.createBuffer(4 * npix, "mesh depth"), dev.createBuffer(4 * npix, "mesh face image")
        rasterizer, visibility = ops.MeshRasterizer(dev), ops.FaceVisibility(dev)
        totals: list = []
        try:
            visibility.reset(F)
            if sizes:   # (grown once, to the largest view, in front of the loop)
                w, h = max(sizes, key=lambda s: s[0] * s[1])
                rasterizer.encode(vertices, V, faces, F, None, bufs[ids[0]], w, h, near, cull, depth=depth, face=image)

            def restart():
                visibility.reset(F)
                totals.clear()

            def measure(i, v, s, w, h):
                s.rasterizer.encodeDepth(None, (depthKind, "weight_sum"))
                rasterizer.encode(vertices, V, faces, F, None, bufs[v], w, h, near, cull, depth=depth, face=image)
                visibility.accumulate(image, w, h, depth, s.rasterizer.getDepthTextureView(depthKind), s.rasterizer.getDepthTextureView("weight_sum"), minWeightSum,
                                      threshold)
                totals.append(visibility.stats())
            self._render_views(ids, imgs, bufs, measure, restart=restart, what=what)
            dev.synchronize()
        except BaseException:
            visibility.destroy()
            raise
        finally:
            rasterizer.destroy()
            depth.destroy()
            image.destroy()
        return visibility, ids, totals

    @staticmethod
    def _per_view(totals: list) -> dict:
        """The cumulative totals as per-view lists: the counted, agreeing and foreign pixels of each view."""
        out = {}
        for name, key in (("counted", "countedPixels"), ("agreeing", "agreeingPixels"), ("foreign", "foreignPixels")):
            cumulative = [0] + [t[key] for t in totals]
            out[name] = [b - a for a, b in zip(cumulative, cumulative[1:])]
        return out

    def meshVisibility(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median", threshold: float = 0.05,
                       minWeightSum: float = 0.5, near: float = ops.MESH_RASTER_NEAR, cull: str = "none") -> dict:
        """Which faces of ``mesh`` (``ops.rasterizeMesh``'s: numpy or a dict of ``HipBuffer``) the views see, and where the model agrees with them: per
        view the mesh is rasterized under the view's camera and its face image accumulated (``ops.FaceVisibility``) beside the mesh's depth and the
        model's ``depthKind`` depth map.  ``dict(iteration, views, counters u32[F,3] = {pixels, agreeing, views}, counted=[...], agreeing=[...],
        foreign=[...], ms)``: per face the pixels that show it over all views, those of them where the model's depth is present (its weight sum at least
        ``minWeightSum``) and within ``threshold`` of the mesh's, and the views that show it; per view the pixels counted, agreeing, and foreign (none,
        for a face image of the same mesh).  ``ops.selectFaces`` turns the counters into a mask and ``ops.filterFaces`` applies it; ``cullMesh`` does
        both on the device.  Where ``meshDepthAgreement`` says how far a mesh disagrees with the model, this says which faces do.

        Rendered through evaluate's passes, with its isolation: the pipeline is drained, a view whose lists overflowed is rendered again (the counters
        are reset and every view is accumulated again), no RNG draw, no training pass, no recording dropped.  Per rank with ``world_size > 1``."""
        t0 = time.perf_counter()
        vertices, faces, V, F, own = ops._mesh_on_device(self.device, mesh, "meshVisibility")
        visibility = None
        try:
            visibility, ids, totals = self._face_visibility("meshVisibility", vertices, faces, V, F, viewIds, split, depthKind, threshold, minWeightSum, near, cull)
            counters = visibility.read()
        finally:
            if visibility is not None:
                visibility.destroy()
            if own:
                vertices.destroy()
                faces.destroy()
        return dict(iteration=self.trainer.iteration, views=ids, counters=counters, **self._per_view(totals), ms=(time.perf_counter() - t0) * 1e3)

    def cullMesh(self, mesh: dict, minPixels: int = 1, minViews: int = 1, minAgreeing: int = 0, minAgreeingFraction: float = 0.0, **visibilityOptions) -> dict:
        """``mesh`` without the faces the views do not see: ``meshVisibility(mesh, **visibilityOptions)``'s counters, ``ops.selectFaces``' rule on them and
        ``ops.filterFaces``, with flags and compaction on the device -- the mesh crosses the bus once each way and not between counters and compaction.
        Returns ``filterFaces``' dict (``vertices``, ``faces``, ``vertexMap``, ``faceMap``, ``invalidFaces``, and ``colours`` / ``keys`` gathered through
        ``vertexMap`` when a numpy mesh has them) with ``counters u32[F,3]``, the counters of the input's faces, and ``views`` added.  With the defaults
        a face stays when at least one pixel of one view shows it; ``minAgreeingFraction`` drops faces the model's depth contradicts.  ``meshVisibility``'s
        isolation."""
        dev = self.device
        defaults = dict(viewIds=None, split="train", depthKind="median", threshold=0.05, minWeightSum=0.5, near=ops.MESH_RASTER_NEAR, cull="none")
        unknown = sorted(set(visibilityOptions) - set(defaults))
        if unknown:
            raise TypeError(f"cullMesh: unknown options {unknown} (meshVisibility's: {sorted(defaults)})")
        opt = dict(defaults, **visibilityOptions)
        ops.selectFaces(np.zeros((0, 3), np.uint32), minPixels, minViews, minAgreeing, minAgreeingFraction)   # (the rule is checked before anything is rendered)
        vertices, faces, V, F, own = ops._mesh_on_device(dev, mesh, "cullMesh")
        visibility = keep = None
        try:
            visibility, ids, _ = self._face_visibility("cullMesh", vertices, faces, V, F, opt["viewIds"], opt["split"], opt["depthKind"], opt["threshold"],
                                                       opt["minWeightSum"], opt["near"], opt["cull"])
            keep = dev.createBuffer(max(F, 1), "face keep flags")
            visibility.flags(keep, minPixels, minViews, minAgreeing, minAgreeingFraction)
            out = ops.filterFaces(dev, dict(vertices=vertices, faces=faces, numVertices=V, numFaces=F), keep)
            out["counters"] = visibility.read()
            out["views"] = ids
        finally:
            for o in (visibility, keep):
                if o is not None:
                    o.destroy()
            if own:
                vertices.destroy()
                faces.destroy()
        for name in ("colours", "keys"):
            if name in mesh and not isinstance(mesh[name], ops.HipBuffer):
                out[name] = None if mesh[name] is None else np.ascontiguousarray(np.asarray(mesh[name])[out["vertexMap"]])
        return out

    # ------------------------------------------------------------------ vertex colours from the photographs
    def bakeMeshColours(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", **options) -> dict:
        """``mesh`` (``ops.bakeVertexColours``': numpy or a dict of ``HipBuffer``) with its vertex colours taken from the split's photographs -- the device
        copies the trainer holds, ``images[v]["texture"]`` -- under the split's cameras: ``ops.bakeVertexColours`` with its ``options`` (``normals``,
        ``depthTolerance``, ``minCos``, ``minViews``, ``minWeight``, ``near``, ``occlusion``, ``asBuffers``) and its result, with ``views`` added.  The views
        may differ in size.  Where a mesh's colours so far are the model's rendered colours averaged into voxels, these are the photographs' own.

        Nothing is rendered through the model: the pipeline is drained and that is all -- no RNG draw, no training pass, no recording dropped, the
        iteration counter untouched.  Per rank with ``world_size > 1``."""
        known = ("normals", "depthTolerance", "minCos", "minViews", "minWeight", "near", "occlusion", "asBuffers")
        unknown = sorted(set(options) - set(known))
        if unknown:
            raise TypeError(f"bakeMeshColours: unknown options {unknown} (bakeVertexColours': {sorted(known)})")
        cams, imgs, bufs, ids = self._views("bakeMeshColours", viewIds, split)
        self._drain()
        views = [(bufs[v], imgs[v]["texture"], int(imgs[v]["width"]), int(imgs[v]["height"])) for v in ids]
        out = ops.bakeMeshFromViews(self.device, mesh, views, what="bakeMeshColours", **options)
        out["views"] = ids
        return out

    # ------------------------------------------------------------------ a texture atlas from the photographs
    def bakeMeshTexture(self, mesh: dict, viewIds: Optional[list] = None, split: str = "train", **options) -> dict:
        """``mesh`` with a texture atlas taken from the split's photographs under the split's cameras: ``ops.bakeTexture`` over the device copies the
        trainer holds, with its ``options`` (``cell``, ``depthTolerance``, ``minCos``, ``minWeight``, ``near``, ``occlusion``, ``twoSided``, ``fill``,
        ``asBuffers``) and its result -- ``texture``, ``uv``, ``texelState``, ``textureStats`` and the atlas's sizes added to the mesh dict -- with ``views``
        added.  The views may differ in size.  ``loaders.saveMeshOBJ`` writes the result.

        Nothing is rendered through the model, as with ``bakeMeshColours``: the pipeline is drained and that is all."""
        known = ("cell", "depthTolerance", "minCos", "minWeight", "near", "occlusion", "twoSided", "fill", "asBuffers")
        unknown = sorted(set(options) - set(known))
        if unknown:
            raise TypeError(f"bakeMeshTexture: unknown options {unknown} (bakeTexture's: {sorted(known)})")
        cams, imgs, bufs, ids = self._views("bakeMeshTexture", viewIds, split)
        self._drain()
        views = [(bufs[v], imgs[v]["texture"], int(imgs[v]["width"]), int(imgs[v]["height"])) for v in ids]
        out = ops.bakeTextureFromViews(self.device, mesh, views, what="bakeMeshTexture", **options)
        out["views"] = ids
        return out

    # ------------------------------------------------------------------ TSDF fusion and mesh extraction
    def fuseDepth(self, volume: ops.TSDFVolume, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median") -> list:
        """Fuses the current model's depth maps into ``volume``: for each view in the order given, the forward pass, rasterize,
        ``encodeDepth((depthKind, "weight_sum"))`` and ``volume.integrate`` with the weight sum and the rasterizer's output texture as colour (where the
        volume has colour).  Returns the view list.

        Rendered through evaluate's passes, with its isolation: the pipeline is drained, no RNG draw, no training pass, no recording dropped, the
        iteration counter untouched.  A view is integrated only once its render is known not to have overflowed its tile-entry lists (one wait per view):
        a fusion cannot be taken back, so it never sees a truncated render.  Per rank with ``world_size > 1``."""
        if depthKind not in ("median", "expected"):
            raise ValueError(f"fuseDepth: depthKind must be 'median' or 'expected', not {depthKind!r}")
        cams, imgs, bufs, ids = self._views("fuseDepth", viewIds, split)
        self._drain()
        for v in ids:
            self._render_views([v], imgs, bufs, lambda i, v, s, w, h: None, what="fuseDepth")   # (returns with the view's complete frame in its pass set)
            w, h = int(imgs[v]["width"]), int(imgs[v]["height"])
            rast = self._set(w, h, bufs[v]).rasterizer
            rast.encodeDepth(None, (depthKind, "weight_sum"))
            volume.integrate(rast.getDepthTextureView(depthKind), bufs[v], w, h, weightSum=rast.getDepthTextureView("weight_sum"),
                             colour=rast.getOutputTextureView() if volume.colour else None)
        return ids

    def extractMesh(self, lo, hi, voxelSize: float, viewIds: Optional[list] = None, split: str = "train", depthKind: str = "median", minWeight: float = 1.0,
                    keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0, weld: str = "host", simplify: Optional[float] = None,
                    smooth: Optional[int] = None, normals: bool = False, cull: Optional[dict] = None, bake=None, texture=None, **volumeOptions) -> dict:
        """The current model as a triangle mesh of the box ``[lo, hi]``: ``ops.TSDFVolume.fromBounds(lo, hi, voxelSize, **volumeOptions)``,
        ``fuseDepth`` over the views, ``extractMesh(minWeight)``; the volume is destroyed.  ``loaders.saveMeshPLY`` writes the result.

        ``keepLargest``, ``minTriangles``, ``minFraction``: with any of them set, the mesh goes through ``ops.removeSmallComponents`` -- the floaters of
        a fused mesh are small components of their own -- and its dict is returned (``vertexMap``, ``faceMap`` and ``components`` added).  With the
        defaults the raw level set is returned as before and nothing more is launched.

        ``weld="device"``: the triangles are welded where the volume emitted them (``ops.weldTrianglesDevice``) and, with a
        component rule, labelled, selected and compacted there as well; the compacted mesh is what is read, and ``colours`` and ``keys`` are read at
        the welded mesh's size and gathered through ``vertexMap``.  The same bytes as ``weld="host"`` either way.

        ``simplify=cellSize``: the mesh is simplified last -- after welding and component removal, so that floaters are not
        merged into the surface first -- by ``ops.simplifyMesh`` on the grid of that cell size from the volume's ``lo``, and its dict is returned
        (``vertices``, ``faces``, ``colours``, ``keys``, ``faceMap``, ``vertexCluster``, ``stats``).  With ``weld="device"`` positions and faces stay
        on the device from the volume to the simplified mesh; with a component rule the colours alone are gathered through ``vertexMap`` on the
        host, 4 bytes per vertex.  The same bytes as ``weld="host"`` either way.  ``None``: as before, and nothing more is launched.

        ``smooth=iterations`` and ``normals=True``: ``ops.smoothMesh`` with its defaults after welding and component removal
        and BEFORE ``simplify`` -- the fine mesh is denoised, then decimated -- with ``stats`` added; and ``normals f32[V,3]``, ``ops.vertexNormals`` of
        the final mesh.  With ``weld="device"`` the positions stay on the device through both.  ``None`` and ``False``: as before, no new key and
        nothing more launched.

        ``cull=dict(...)``: the faces no view sees are removed by ``cullMesh(mesh, **cull)`` -- its rule (``minPixels``,
        ``minViews``, ``minAgreeing``, ``minAgreeingFraction``) and ``meshVisibility``'s options, with ``viewIds``, ``split`` and ``depthKind`` defaulting
        to the extraction's own -- after welding and component removal and BEFORE ``smooth``, ``simplify`` and ``normals``, which see the boundary it
        cuts; ``cullMesh``'s dict is what goes on (``vertexMap`` and ``faceMap`` are its own, into the mesh it was given).  The welded mesh is read and
        handed to ``cullMesh`` as numpy with either weld, so the bytes are the same.  ``None``: as before, no new key and nothing more launched.

        ``bake=True`` or ``bake=dict(...)``: the final mesh -- after ``simplify`` -- gets its vertex colours from the photographs by
        ``bakeMeshColours(mesh, **bake)``, with ``viewIds`` and ``split`` defaulting to the extraction's own; ``colours`` is replaced and ``baked``,
        ``bakeStats`` (the baker's totals; ``stats`` stays the smoother's or the simplifier's) and ``views`` are added.  The weights are the final mesh's vertex normals, computed
        for that even when ``normals=False`` (no ``normals`` key is added then).  ``None``: as before, no new key and nothing more launched.

        ``texture=True`` or ``texture=dict(...)``: last of all -- after ``bake`` -- the mesh gets a texture atlas from the photographs
        by ``bakeMeshTexture(mesh, **texture)``, with ``viewIds`` and ``split`` defaulting to the extraction's own; ``texture``, ``uv``, ``texelState``,
        ``textureStats``, ``textureWidth``, ``textureHeight``, ``textureCell`` and ``views`` are added and no other key changes.  ``None``: as before, no new
        key and nothing more launched."""
        if weld not in ("host", "device"):
            raise ValueError(f"extractMesh: weld must be 'host' or 'device', not {weld!r}")
        if texture is not None and texture is not False:
            mesh = self.extractMesh(lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld=weld, simplify=simplify,
                                    smooth=smooth, normals=normals, cull=cull, bake=bake, **volumeOptions)
            return self.bakeMeshTexture(mesh, **dict(dict(viewIds=viewIds, split=split), **({} if texture is True else texture)))
        if bake is not None and bake is not False:
            mesh = self.extractMesh(lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld=weld, simplify=simplify,
                                    smooth=smooth, normals=normals, cull=cull, **volumeOptions)
            out = self.bakeMeshColours(mesh, **dict(dict(viewIds=viewIds, split=split), **({} if bake is True else bake)))
            out["bakeStats"] = out.pop("stats")
            if "stats" in mesh:
                out["stats"] = mesh["stats"]
            return out
        if cull is not None:
            mesh = self.extractMesh(lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld=weld, **volumeOptions)
            culled = self.cullMesh(mesh, **dict(dict(viewIds=viewIds, split=split, depthKind=depthKind), **cull))
            return ops.finishMesh(self.device, culled, np.asarray(lo, np.float64).reshape(3).astype(np.float32), smooth, simplify, normals)
        if simplify is not None or smooth is not None or normals:
            return self._extract_finished(lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld, simplify,
                                          smooth, normals, volumeOptions)
        everything = ops._is_default_selection(keepLargest, minTriangles, minFraction)
        volume = ops.TSDFVolume.fromBounds(self.device, lo, hi, voxelSize, **volumeOptions)
        mesh = welded = None
        try:
            self.fuseDepth(volume, viewIds, split, depthKind)
            if weld == "host" or everything:
                mesh = volume.extractMesh(minWeight, weld=weld)
            else:
                tri = volume.extractTriangleBuffers(minWeight)
                try:
                    welded = ops.weldTrianglesDevice(self.device, tri, asBuffers=True)
                finally:
                    ops.destroyBuffers(tri)
        finally:
            volume.destroy()
        if everything:
            return mesh
        if welded is None:
            return ops.removeSmallComponents(self.device, mesh, keepLargest, minTriangles, minFraction)
        try:
            out = ops.removeSmallComponents(self.device, dict(vertices=welded["vertices"], faces=welded["faces"]), keepLargest, minTriangles, minFraction)
            V = welded["numVertices"]
            out["colours"] = None if welded["colours"] is None else np.ascontiguousarray(
                welded["colours"].read(np.uint8, count=4 * V).reshape(V, 4)[:, :3][out["vertexMap"]])
            out["keys"] = np.ascontiguousarray(welded["keys"].read(np.uint64, count=V)[out["vertexMap"]])
            return out
        finally:
            ops.destroyBuffers(welded)

    def _extract_finished(self, lo, hi, voxelSize, viewIds, split, depthKind, minWeight, keepLargest, minTriangles, minFraction, weld, simplify, smooth, normals,
                          volumeOptions) -> dict:
        """``extractMesh`` with ``simplify``, ``smooth`` or ``normals`` set: volume, weld, component removal (when a rule is given), then
        ``ops.finishMesh``: smoothing, simplification from the volume's origin, normals."""
        everything = ops._is_default_selection(keepLargest, minTriangles, minFraction)
        volume = ops.TSDFVolume.fromBounds(self.device, lo, hi, voxelSize, **volumeOptions)
        welded, kept = {}, {}
        try:
            self.fuseDepth(volume, viewIds, split, depthKind)
            origin = volume.origin
            if everything:
                return volume.extractMesh(minWeight, weld=weld, simplify=simplify, smooth=smooth, normals=normals)
            if weld == "host":
                mesh = ops.removeSmallComponents(self.device, volume.extractMesh(minWeight), keepLargest, minTriangles, minFraction)
                return ops.finishMesh(self.device, mesh, origin, smooth, simplify, normals)
            tri = volume.extractTriangleBuffers(minWeight)
            try:
                welded = ops.weldTrianglesDevice(self.device, tri, asBuffers=True)
            finally:
                ops.destroyBuffers(tri)
            kept = ops.removeSmallComponents(self.device, dict(vertices=welded["vertices"], faces=welded["faces"]), keepLargest, minTriangles, minFraction,
                                             asBuffers=True)
            V, nv, nf = welded["numVertices"], kept["numVertices"], kept["numFaces"]
            if simplify is not None and welded["colours"] is not None:
                gathered = welded["colours"].read(np.uint32, count=V)[kept["vertexMap"].read(np.uint32, count=nv)]
                kept["colours"] = self.device.bufferFrom(np.ascontiguousarray(gathered), "compacted colours")

            def read(b) -> dict:   # what removeSmallComponents returns for the numpy mesh: colours and keys gathered through vertexMap
                out = dict(vertices=b["vertices"].read(np.float32, count=3 * nv).reshape(nv, 3), faces=b["faces"].read(np.uint32, count=3 * nf).reshape(nf, 3),
                           vertexMap=b["vertexMap"].read(np.uint32, count=nv), faceMap=b["faceMap"].read(np.uint32, count=nf), components=b["components"])
                out["colours"] = None if welded["colours"] is None else np.ascontiguousarray(
                    welded["colours"].read(np.uint8, count=4 * V).reshape(V, 4)[:, :3][out["vertexMap"]])
                out["keys"] = np.ascontiguousarray(welded["keys"].read(np.uint64, count=V)[out["vertexMap"]])
                return out

            return ops.finishMesh(self.device, kept, origin, smooth, simplify, normals, read)
        finally:
            volume.destroy()
            ops.destroyBuffers(welded)
            ops.destroyBuffers(kept)

    # ------------------------------------------------------------------ mesh accuracy against a reference point set
    def evaluateGeometry(self, reference, lo, hi, voxelSize: float, maxDistance: float, threshold: float, density: Optional[float] = None, seed: int = 0,
                         keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0, **extractMeshOptions) -> dict:
        """Scores the current model's geometry against ``reference`` -- an ``[M,3]`` array of surface points, or the path of a PLY that holds them:
        ``extractMesh(lo, hi, voxelSize, **extractMeshOptions)``, ``ops.sampleMesh`` at ``density`` samples per unit area (``None``: ``1 / (voxelSize / 2)^2``,
        a spacing of half a voxel) and ``ops.geometryMetrics(samples, reference, maxDistance, threshold)``.  Returns its dict -- accuracy, completeness,
        chamfer, precision, recall, fscore and the counts -- with ``vertices``, ``faces``, ``samples`` (the mesh's and the sample count) and ``ms``.

        ``keepLargest``, ``minTriangles`` and ``minFraction`` are ``extractMesh``'s: the published numbers are those of a mesh without its floaters.

        ``extractMesh``'s isolation (``fuseDepth``'s): the pipeline is drained, no RNG draw, no training pass, no recording dropped, the iteration counter
        untouched.  No alignment is attempted: the reference is taken to be in the scene's frame."""
        t0 = time.perf_counter()
        ref = loaders.loadPointsPLY(reference) if isinstance(reference, (str, bytes)) or hasattr(reference, "__fspath__") else np.ascontiguousarray(reference, np.float32)
        if ref.ndim != 2 or ref.shape[1] != 3:
            raise ValueError(f"evaluateGeometry: the reference must be [M, 3] points, got {ref.shape}")
        if density is None:
            density = 1.0 / (0.5 * float(voxelSize)) ** 2
        mesh = self.extractMesh(lo, hi, voxelSize, keepLargest=keepLargest, minTriangles=minTriangles, minFraction=minFraction, **extractMeshOptions)
        samples = ops.sampleMesh(self.device, mesh, density, seed, asBuffers=True)
        try:
            n = samples["count"]
            out = ops.geometryMetrics(self.device, self.device.view(samples["points"].ptr, 12 * n), ref, maxDistance, threshold)
        finally:
            samples["points"].destroy()
            samples["face"].destroy()
        out.update(vertices=int(mesh["vertices"].shape[0]), faces=int(mesh["faces"].shape[0]), samples=int(n), ms=(time.perf_counter() - t0) * 1e3)
        return out

    # ------------------------------------------------------------------ render contribution
    def contributionBuffer(self, viewIds: Optional[list], split: str, what: str) -> tuple:
        """(buffer, view ids): the views' contribution records accumulated into one new device buffer (``Trainer.pruneByContribution`` decides on it)."""
        cams, imgs, bufs, ids = self._views(what, viewIds, split)
        if sum(int(imgs[v]["width"]) * int(imgs[v]["height"]) for v in ids) >= 2 ** 32:
            raise ValueError(f"{what}: the views hold 2^32 pixels or more; the per-Gaussian pixel count is 32 bits wide")
        self._drain()
        stats = ops.createContributionBuffer(self.device, self.trainer.pointCloud.num_points)
        try:
            self._render_views(ids, imgs, bufs, lambda i, v, s, w, h: s.rasterizer.encodeContribution(None, stats), restart=stats.clear, what=what)
        except BaseException:
            stats.destroy()
            raise
        return stats, ids

    def contributionStats(self, viewIds: Optional[list] = None, split: str = "train") -> dict:
        """How much of each Gaussian the views' images hold: ``dict(sum_q, weight_sum, max_weight, pixels, views)``, one
        entry per Gaussian, accumulated over the views -- the sum and the maximum of the compositing weights ``alpha (1 - A)`` and the number of
        (pixel, Gaussian) pairs composited.  Rendered through evaluate's passes, with its isolation: the pipeline is drained, a view whose lists
        overflowed is rendered again (the records are cleared and every view is walked again), no RNG draw, no training pass, no recording
        dropped.  Per rank with ``world_size > 1``."""
        stats, ids = self.contributionBuffer(viewIds, split, "contributionStats")
        try:
            out = ops.readContribution(stats, self.trainer.pointCloud.num_points)
        finally:
            stats.destroy()
        out["views"] = ids
        return out
