"""Preview path: forward pass + rasterizer + blit, mirroring ``src/viewer.ts:8-115`` without the browser.

The reference's ``Viewer`` owns a ``Camera`` bound to a canvas, builds a ``TiledForwardPass`` in ``'pointcloud'`` render mode
and a ``TiledRasterizer`` on ``setPointCloud`` (viewer.ts:46-66), and per frame encodes forward -> rasterize ->
``blitToTexture(swapChainView)`` (viewer.ts:72-87).  Here the canvas is a ``width x height`` rgba8 device buffer (the
"swap-chain image"); ``readFrame`` / ``savePNG`` take the place of presentation.  Camera interaction (``CameraControl``) is
UI and stays out; the camera is set from a ``CameraData`` dict or a ready 68-float block.
"""
from __future__ import annotations

import struct
import zlib
from typing import Optional

import numpy as np

from . import loaders
from .ops import (MESH_RASTER_NEAR, HipBuffer, HipDevice, HipEncoder, PointCloud, TiledForwardPass, TiledRasterizer, depthToRGBA8, faceIndexColours, grownTileEntries,
                  normalToRGBA8, rasterizeMesh)


def encodePNG(rgba: np.ndarray) -> bytes:
    """Minimal PNG writer (8-bit RGBA, filter 0, one IDAT) for ``[H, W, 4]`` uint8 frames."""
    a = np.ascontiguousarray(rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("encodePNG expects an [H, W, 4] uint8 array")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * 4)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


class Camera:
    """``Camera`` (``src/camera/camera.ts:100-205``) without the browser: ``canvas`` is any object with ``width`` and ``height``.  Owns the
    272-byte uniform buffer a forward pass reads and rewrites it, stream-ordered, on every ``update_buffer()``."""

    def __init__(self, canvas, device: HipDevice):
        self.canvas, self.device = canvas, device
        self.uniform_buffer: HipBuffer = device.createBuffer(272, "camera uniform")
        self.uniforms = np.zeros(68, np.float32)
        self.reset()

    def reset(self) -> None:
        """camera.ts:113-119: position (0, 0, 5), identity rotation, fovY 45 degrees."""
        self._preset = dict(position=(0.0, 0.0, 5.0))
        self.on_update_canvas()

    def on_update_canvas(self) -> None:
        self.update_buffer()

    def update_buffer(self) -> None:
        self.uniforms = loaders.cameraUniforms(self._preset, int(self.canvas.width), int(self.canvas.height))
        self.uniform_buffer.write(self.uniforms)

    def set_preset(self, preset: dict) -> None:
        """camera.ts:196-205: a CameraData dict (pose kept where the preset has none; fovY from height and fy when both are there)."""
        merged = dict(self._preset)
        for k in ("position", "rotation"):
            if preset.get(k) is not None:
                merged[k] = preset[k]
        if preset.get("fx") and preset.get("fy") and preset.get("height"):
            merged.update(fx=preset["fx"], fy=preset["fy"], height=preset["height"])
        self._preset = merged
        self.on_update_canvas()


class Viewer:
    """``Viewer`` (``src/viewer.ts``): ``setPointCloud``, ``render(encoder)``, pass-through setters, resize handling."""

    def __init__(self, device: HipDevice, width: int, height: int, format: str = "rgba8unorm"):
        self.device = device
        self.presentationFormat = format
        self.width, self.height = int(width), int(height)
        self.forwardPass: Optional[TiledForwardPass] = None
        self.rasterizer: Optional[TiledRasterizer] = None
        self.pointCloud: Optional[PointCloud] = None
        self._camera_data: Optional[dict] = None
        self.cameraBuffer: HipBuffer = device.createBuffer(272, "camera uniforms")
        self.frameBuffer: HipBuffer = device.createBuffer(4 * self.width * self.height, "swap-chain image")
        self.setCamera(dict(position=(0.0, 0.0, 5.0)))  # Camera defaults (camera.ts:113-136)

    # ---- camera (camera.ts:138-205 via loaders.cameraUniforms)
    def setCamera(self, camera) -> None:
        """``camera``: a CameraData dict (``loaders.loadCameraJson`` / ``mergeColmap`` entries) or 68 floats."""
        if isinstance(camera, dict):
            self._camera_data = camera
            block = loaders.cameraUniforms(camera, self.width, self.height)
        else:
            self._camera_data = None
            block = np.asarray(camera, np.float32).reshape(68)
        self.cameraBuffer.write(block)

    def setPointCloud(self, pointCloud: PointCloud) -> None:
        self._settings = dict(renderMode="pointcloud")  # (viewer.ts:46-66: a new cloud starts in point-cloud mode, default scale and point size)
        self._tile_entries = 0
        self.pointCloud = pointCloud
        self._build_passes()

    def _build_passes(self) -> None:
        if self.forwardPass is not None:
            self.forwardPass.destroy()
        if self.rasterizer is not None:
            self.rasterizer.destroy()
        self.forwardPass = TiledForwardPass(self.device, self.pointCloud, self.cameraBuffer,
                                            dict(viewportWidth=self.width, viewportHeight=self.height, renderMode="pointcloud", maxTileEntries=self._tile_entries))
        self.rasterizer = TiledRasterizer(dict(device=self.device, forwardPass=self.forwardPass, format=self.presentationFormat))
        for k, apply in (("renderMode", self.forwardPass.setRenderMode), ("gaussianScale", self.forwardPass.setGaussianScale), ("pointSize", self.forwardPass.setPointSize)):
            if k in self._settings:
                apply(self._settings[k])

    def update(self, dt: float) -> None:
        """Camera-control integration step of the reference (viewer.ts:68-70); no interactive control here."""

    def render(self, commandEncoder: Optional[HipEncoder] = None) -> None:
        if self.forwardPass is None or self.rasterizer is None or self.pointCloud is None:
            return
        self.forwardPass.encode(commandEncoder)
        self.rasterizer.encode(commandEncoder, self.width, self.height)
        self.rasterizer.blitToTexture(commandEncoder, self.frameBuffer, self.width, self.height)

    # ---- pass-through setters / getters (viewer.ts:89-104)
    def setRenderMode(self, mode: str) -> None:
        if self.forwardPass is not None:
            self._settings["renderMode"] = mode
            self.forwardPass.setRenderMode(mode)

    def setGaussianScale(self, value: float) -> None:
        if self.forwardPass is not None:
            self._settings["gaussianScale"] = value
            self.forwardPass.setGaussianScale(value)

    def setPointSize(self, value: float) -> None:
        if self.forwardPass is not None:
            self._settings["pointSize"] = value
            self.forwardPass.setPointSize(value)

    def getForwardPass(self) -> Optional[TiledForwardPass]:
        return self.forwardPass

    def resize(self, width: int, height: int) -> None:
        """``handleResize`` (viewer.ts:106-113): new canvas size -> camera block and forward-pass viewport follow."""
        self.width, self.height = int(width), int(height)
        self.frameBuffer.destroy()
        self.frameBuffer = self.device.createBuffer(4 * self.width * self.height, "swap-chain image")
        if self._camera_data is not None:
            self.cameraBuffer.write(loaders.cameraUniforms(self._camera_data, self.width, self.height))
        if self.forwardPass is not None:
            self.forwardPass.setViewport(self.width, self.height)

    # ---- presentation
    def _settle_capacity(self, rerender) -> None:
        """Waits for this viewer's frame.  If its tile-entry list outran what the library sized for the cloud (the reference would show the truncated
        picture; the library reports it), the viewer's passes are rebuilt around larger lists and ``rerender()`` encodes the frame again.  (A report
        about this viewer's pass may have been consumed by another owner's wait -- a Trainer on the same device: it was left in
        ``device.capacityReports``, and ``settle`` finds it there.)"""
        for _ in range(4):  # this viewer's own pass: its word is consumed by its own check
            if self.forwardPass is None:
                break
            mine = self.device.capacityReports.settle([int(self.forwardPass.handle.value or 0)], self.forwardPass.check).mine
            if not mine:
                break
            self._tile_entries = grownTileEntries(mine[0].capacity, mine[0].needed)
            self._build_passes()
            rerender()

    def readFrame(self) -> np.ndarray:
        """The presented image as ``[H, W, 4]`` uint8 (synchronises; a frame whose tile-entry list outran the passes is rendered again around
        larger ones, ``_settle_capacity``)."""
        self._settle_capacity(lambda: self.render(None))
        return self.frameBuffer.read(np.uint8, 4 * self.width * self.height).reshape(self.height, self.width, 4)

    # ---- depth (no reference counterpart)
    def _encode_depth(self, kind: str) -> None:
        self.forwardPass.setRenderMode("gaussian")   # depth has weights in gaussian mode only; the viewer's own mode is put back below
        try:
            self.forwardPass.encode(None)
            self.rasterizer.encode(None, self.width, self.height)
            self.rasterizer.encodeDepth(None, (kind,))
        finally:
            self.forwardPass.setRenderMode(self._settings.get("renderMode", "pointcloud"))

    def renderDepth(self, kind: str = "expected") -> np.ndarray:
        """The current camera's depth image ``[H, W]`` float32 (``ops.DEPTH_KINDS``), rendered in gaussian mode through the viewer's own passes
        whatever its render mode, which is left as it was (synchronises).  The swap-chain image is not touched; the passes' colour images hold the
        gaussian-mode frame afterwards, until the next ``render``."""
        if self.forwardPass is None or self.rasterizer is None or self.pointCloud is None:
            raise RuntimeError("Viewer.renderDepth: no point cloud set")
        self._encode_depth(kind)
        self._settle_capacity(lambda: self._encode_depth(kind))
        return self.rasterizer.getDepthTextureView(kind).read(np.float32, self.width * self.height).reshape(self.height, self.width)

    def saveDepthPNG(self, path: str, near: Optional[float] = None, far: Optional[float] = None, kind: str = "expected") -> None:
        """The depth image as a grey PNG (inverse depth, near white, far black, no depth black).  ``near`` / ``far`` default to the smallest / largest
        non-zero depth of the frame."""
        d = self.renderDepth(kind)
        seen = d[np.isfinite(d) & (d > 0)]
        lo = float(near) if near is not None else (float(seen.min()) if seen.size else 1.0)
        hi = float(far) if far is not None else (float(seen.max()) if seen.size else 2.0)
        if not hi > lo:   # (one depth only: any range around it)
            hi = float(np.nextafter(np.float32(lo), np.float32(np.inf))) * 2.0
        out = self.device.createBuffer(4 * self.width * self.height, "depth presentation")
        try:
            depthToRGBA8(self.device, self.rasterizer.getDepthTextureView(kind), self.width, self.height, lo, hi, out)
            rgba = out.read(np.uint8, 4 * self.width * self.height).reshape(self.height, self.width, 4)
        finally:
            out.destroy()
        with open(path, "wb") as f:
            f.write(encodePNG(rgba))

    # ---- normals (no reference counterpart)
    def _encode_normal(self) -> None:
        self.forwardPass.setRenderMode("gaussian")   # as depth: weights exist in gaussian mode only; the viewer's own mode is put back below
        try:
            self.forwardPass.encode(None)
            self.rasterizer.encode(None, self.width, self.height)
            self.rasterizer.encodeNormal(None)
        finally:
            self.forwardPass.setRenderMode(self._settings.get("renderMode", "pointcloud"))

    def renderNormals(self) -> np.ndarray:
        """The current camera's normal map ``[H, W, 4]`` float32 ``{N.x, N.y, N.z, A}`` (view space: x right, y down, z forward; ``N`` un-normalised,
        ``|N| <= A``), rendered in gaussian mode through the viewer's own passes whatever its render mode, which is left as it was (synchronises).
        The swap-chain image is not touched."""
        if self.forwardPass is None or self.rasterizer is None or self.pointCloud is None:
            raise RuntimeError("Viewer.renderNormals: no point cloud set")
        self._encode_normal()
        self._settle_capacity(self._encode_normal)
        return self.rasterizer.getNormalTextureView().read(np.float32, 4 * self.width * self.height).reshape(self.height, self.width, 4)

    def saveNormalPNG(self, path: str) -> None:
        """The normal map as the usual colour PNG (``ops.normalToRGBA8``: a surface that faces the camera is blue, no normal black)."""
        self.renderNormals()
        out = self.device.createBuffer(4 * self.width * self.height, "normal presentation")
        try:
            normalToRGBA8(self.device, self.rasterizer.getNormalTextureView(), self.width, self.height, out)
            rgba = out.read(np.uint8, 4 * self.width * self.height).reshape(self.height, self.width, 4)
        finally:
            out.destroy()
        with open(path, "wb") as f:
            f.write(encodePNG(rgba))

    # ---- meshes (no reference counterpart)
    def renderMesh(self, mesh: dict, mode: str = "colour", near: float = MESH_RASTER_NEAR, cull: str = "none", depthRange: Optional[tuple] = None) -> np.ndarray:
        """``mesh`` (``ops.rasterizeMesh``'s: numpy or a dict of ``HipBuffer``) under the current camera as ``[H, W, 4]`` uint8, alpha 255 where a face
        shows and the pixel all zero -- black -- where none does, except as the presentation kernels say: ``"colour"``, the interpolated vertex
        colours; ``"depth"``, ``ops.depthToRGBA8`` between ``depthRange`` (default: the smallest and largest depth of the image); ``"normal"``,
        ``ops.normalToRGBA8`` of the faces' geometric normals; ``"face"``, a fixed integer hash of the face index.  Needs no point cloud and touches
        neither the swap-chain image nor the viewer's passes (synchronises)."""
        if mode not in ("colour", "depth", "normal", "face"):
            raise ValueError(f"Viewer.renderMesh: mode must be 'colour', 'depth', 'normal' or 'face', not {mode!r}")
        w, h = self.width, self.height
        if mode in ("colour", "face"):
            out = rasterizeMesh(self.device, mesh, self.cameraBuffer, w, h, near, cull, (mode,))
            return out["colour"] if mode == "colour" else faceIndexColours(out["face"])
        bufs = rasterizeMesh(self.device, mesh, self.cameraBuffer, w, h, near, cull, (mode,), asBuffers=True)
        target = self.device.createBuffer(4 * w * h, "mesh presentation")
        try:
            if mode == "depth":
                lo, hi = depthRange if depthRange is not None else (None, None)
                if lo is None or hi is None:
                    d = bufs["depth"].read(np.float32, w * h)
                    seen = d[d > 0]
                    lo = float(seen.min()) if lo is None and seen.size else (1.0 if lo is None else float(lo))
                    hi = float(seen.max()) if hi is None and seen.size else (2.0 if hi is None else float(hi))
                if not hi > lo:   # (one depth only: any range around it)
                    hi = float(np.nextafter(np.float32(lo), np.float32(np.inf))) * 2.0
                depthToRGBA8(self.device, bufs["depth"], w, h, lo, hi, target)
            else:
                normalToRGBA8(self.device, bufs["normal"], w, h, target)
            return target.read(np.uint8, 4 * w * h).reshape(h, w, 4)
        finally:
            target.destroy()
            bufs[mode].destroy()

    def saveMeshPNG(self, path: str, mesh: dict, mode: str = "colour", **options) -> None:
        """``renderMesh(mesh, mode, **options)`` as a PNG."""
        with open(path, "wb") as f:
            f.write(encodePNG(self.renderMesh(mesh, mode, **options)))

    def savePNG(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(encodePNG(self.readFrame()))

    def destroy(self) -> None:
        if self.forwardPass is not None:
            self.forwardPass.destroy()
        if self.rasterizer is not None:
            self.rasterizer.destroy()
        self.forwardPass = self.rasterizer = None
