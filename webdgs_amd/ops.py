"""Host-side mirror of the reference's operator classes over the C ABI (``include/webdgs.h``).

Class and method names follow ``/root/reference/src/renderers/*.ts``, ``src/sort/sort_dynamic.ts``,
``src/prefix/prefix.ts`` and ``src/utils/allocate-pointcloud.ts`` so that code shaped like
``src/trainer.ts`` drives them unchanged; ``GPUDevice / GPUBuffer / GPUTextureView / GPUCommandEncoder`` become
``HipDevice / HipBuffer / HipEncoder``.  PyTorch appears only as the allocator for caller-owned device memory
(point clouds, cameras, images, optimizer state) and as the owner of the HIP stream; every kernel is in
``libwebdgs_hip.so``.  There is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import CapacityError, StateError, WdgsError, check  # noqa: F401  (re-exported)


# ----------------------------------------------------------------------------- device / buffers
MAX_LANES = 4  # WDGS_MAX_LANES (include/webdgs.h)
MAX_BATCH_VIEWS = 16  # WDGS_MAX_BATCH_VIEWS


class HipBuffer:
    """A span of device memory (``GPUBuffer``): either a view into library-owned memory or a torch-backed allocation."""

    def __init__(self, device: "HipDevice", ptr: int, size: int, owner: Optional[torch.Tensor] = None, label: str = ""):
        self.device, self.ptr, self.size, self._owner, self.label = device, int(ptr or 0), int(size), owner, label
        self.destroyed = False
        # called before the buffer's CONTENT is handed to the host (read / tensor): a producer that keeps part of it elsewhere brings it up
        # to date first (the optimizer's deferred SH writes: Optimizer.setDeferredSH)
        self.before_read = None

    def read(self, dtype=np.uint32, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        """mapAsync + getMappedRange: synchronous copy to host."""
        dt = np.dtype(dtype)
        if self.before_read is not None:
            self.before_read()
        n = (self.size - offset) // dt.itemsize if count is None else int(count)
        out = np.empty(n, dt)
        if n:
            check(self.device.lib.wdgs_copy_to_host(self.device.handle, out.ctypes.data, self.ptr + offset, n * dt.itemsize))
        return out

    def write(self, data: np.ndarray, offset: int = 0) -> None:
        """queue.writeBuffer: stream-ordered."""
        a = np.ascontiguousarray(data)
        if a.nbytes + offset > self.size:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"write of {a.nbytes} bytes at {offset} exceeds buffer size {self.size}")
        check(self.device.lib.wdgs_copy_to_device(self.device.handle, self.ptr + offset, a.ctypes.data, a.nbytes))
        self.device._keepalive.append(a)

    def clear(self) -> None:
        check(self.device.lib.wdgs_memset(self.device.handle, self.ptr, 0, self.size))

    def tensor(self) -> torch.Tensor:
        if self._owner is None:
            raise _lib.StateError(_lib.WDGS_E_STATE, "buffer is library-owned; no torch tensor behind it")
        if self.before_read is not None:
            self.before_read()
        return self._owner

    def destroy(self) -> None:
        self.destroyed = True
        self._owner = None


class HipCommandBuffer:
    """``GPUCommandBuffer`` backed by an instantiated HIP graph; unlike WebGPU's it may be submitted repeatedly."""

    def __init__(self, device: "HipDevice", handle):
        self.device, self.handle = device, handle

    def destroy(self) -> None:
        if self.handle:
            self.device.lib.wdgs_command_buffer_destroy(self.handle)
            self.handle = None


class HipEncoder:
    """``GPUCommandEncoder``.  Eager (default): ops enqueue on the device stream as they are encoded and ``finish()`` is a
    marker.  ``record=True``: encodes are captured into a HIP graph; ``finish()`` returns a replayable ``HipCommandBuffer``."""

    def __init__(self, device: "HipDevice", label: str = "", record: bool = False):
        self.device, self.label, self.record = device, label, record
        self._open = False
        if record:
            check(device.lib.wdgs_encoder_begin(device.handle))
            self._open = True

    def __enter__(self) -> "HipEncoder":
        return self

    def __exit__(self, exc_type, exc, tb) -> bool:
        """``with device.createCommandEncoder(record=True) as enc:`` -- an exception inside the block (a failed encode, a
        Python error) drops the recording instead of leaving the device's stream in capture mode."""
        if exc_type is not None:
            self.abort()
        return False

    def abort(self) -> None:
        """Discards an unfinished recording (``wdgs_encoder_abort``); a no-op for eager or finished encoders."""
        if self._open:
            self._open = False
            check(self.device.lib.wdgs_encoder_abort(self.device.handle))

    def clearBuffer(self, buf: HipBuffer) -> None:
        buf.clear()

    def copyBufferToBuffer(self, src: HipBuffer, src_off: int, dst: HipBuffer, dst_off: int, size: int) -> None:
        """``encoder.copyBufferToBuffer`` (trainer.ts:445): device to device, stream-ordered, recordable."""
        if src_off + size > src.size or dst_off + size > dst.size:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"copyBufferToBuffer: {size} bytes at {src_off} -> {dst_off} exceed the buffers ({src.size}, {dst.size})")
        if src.before_read is not None:
            src.before_read()
        check(self.device.lib.wdgs_copy_buffer_to_buffer(self.device.handle, dst.ptr + dst_off, src.ptr + src_off, int(size)))

    def finish(self):
        if not self.record:
            return self
        if not self._open:
            raise _lib.StateError(_lib.WDGS_E_STATE, "encoder already finished or aborted")
        self._open = False  # wdgs_encoder_finish leaves capture mode whether or not it succeeds
        h = C.c_void_p()
        check(self.device.lib.wdgs_encoder_finish(self.device.handle, C.byref(h)))
        return HipCommandBuffer(self.device, h)


class _Queue:
    def __init__(self, device: "HipDevice"):
        self.device = device

    def submit(self, cmds) -> None:
        """Eager encoders have already put their work on the stream; recorded command buffers are launched here."""
        for c in cmds or ():
            if isinstance(c, HipCommandBuffer):
                check(self.device.lib.wdgs_queue_submit(self.device.handle, c.handle))

    def onSubmittedWorkDone(self, callback=None) -> None:
        """Without a callback: block until the stream drains (the awaited Promise of trainer.ts:639-645).  With one: return
        at once; ``callback()`` runs on a runtime thread when the work submitted so far is done (it must not touch the GPU)."""
        if callback is None:
            self.device.synchronize()
            return
        cb = _lib.DoneCallback(lambda _user: callback())
        self.device._keepalive.append(cb)  # the trampoline must outlive its call; released at the next synchronize()
        check(self.device.lib.wdgs_queue_on_done(self.device.handle, cb, None))

    def mark(self) -> int:
        """A ticket for "everything submitted to the current lane so far" -- the Promise of ``onSubmittedWorkDone()``, kept for later."""
        t = C.c_uint64(0)
        check(self.device.lib.wdgs_queue_mark(self.device.handle, C.byref(t)))
        return int(t.value)

    def wait(self, ticket: int) -> None:
        """Awaits a ticket: blocks until that work is done, then raises deferred device-side errors like ``synchronize()``."""
        check(self.device.lib.wdgs_queue_wait(self.device.handle, C.c_uint64(int(ticket))))

    def writeBuffer(self, buf: HipBuffer, offset: int, data: np.ndarray) -> None:
        buf.write(data, offset)


class Overflow(NamedTuple):
    """One pass's line of a capacity report: the entries its frame needed, what its lists hold, the forward pass's handle."""
    needed: int
    capacity: int
    handle: int


class Settled(NamedTuple):
    """What ``CapacityReports.settle`` found for one owner: its passes' lines, whether a line was left for another owner, and the report its lines
    came from (``None`` when there are none)."""
    mine: list
    foreign: bool
    error: Optional[Exception]


def grownTileEntries(now: int, needed: int) -> int:
    """Tile-entry lists after an overflow: twice what they hold, or 1.5 x what the frame needed where that is more; never more than a sort takes."""
    return min(max(2 * now, int(needed * 1.5)), 0xFFFFF000)


class CapacityReports:
    """Capacity reports that reached the wrong owner.  The library reports a truncated tile-entry list at the next host wait on the DEVICE, to whoever
    waits (csrc/api.hip: deferred_checks consumes every pass's word and names up to four passes).  The owners of forward passes on a device -- a
    Trainer's training and metric sets, its Evaluator's sets, a Viewer -- all wait through ``settle``, which has the one rule: an owner keeps the lines
    about its own passes, every other line is left HERE as a report of its own, where the passes' owner finds it at its own next wait (ADVICE r4:
    dropped instead, a report consumed by the wrong owner was lost to the right one)."""

    def __init__(self, keep: int = 16):
        self.pending: list = []
        self.keep = keep

    def settle(self, own_handles, wait) -> Settled:
        """``wait()``, then the capacity report it raised -- or, if that had no line of ``own_handles``' passes, the oldest pending report that has one --
        sorted: the owner's lines are returned, the others posted.  A report that names no pass (an optimizer step skipped on every rank: nobody's)
        and every other error propagate."""
        own = {int(h) for h in own_handles}
        mine, foreign, report = [], False, None
        try:
            wait()
        except CapacityError as e:
            if not self.parse(e):
                raise
            report = e
            mine, foreign = self._keep(report, own)
        if not mine:
            report = self.take(own)
            if report is not None:
                mine, left = self._keep(report, own)
                foreign = foreign or left
        return Settled(mine, foreign, report if mine else None)

    def _keep(self, report, own: set) -> tuple:
        """``split``; the other owners' lines are posted as one report in deferred_checks' format, so that ``parse`` stays the reader of report text."""
        mine, others = self.split(report, own)
        if others:
            lines = "; ".join(f"{o.needed} entries needed, max_tile_entries = {o.capacity} (forward pass {o.handle:#x})" for o in self.parse(report) if o.handle not in own)
            self.post(CapacityError(_lib.WDGS_E_CAPACITY, f"tile entries overflow: {lines} (raise wdgs_tiled_forward_config.max_tile_entries)"))
        return mine, others

    @staticmethod
    def parse(error) -> list:
        """One ``Overflow(needed, capacity, handle)`` per pass the report names, in the report's order; ``[]`` for any other error."""
        # The one reader of report text (bindings/ts/capacity_reports.js has its twin).  It follows two format strings of csrc/api.hip:
        #   deferred_checks:          "tile entries overflow: " + "; ".join("%u entries needed, max_tile_entries = %u (forward pass %p)") + " (raise ...)"
        #   wdgs_tiled_forward_check: "tile entries overflow: %u entries needed, max_tile_entries = %u (forward pass %p)"
        # Known limit: the library names at most four passes per report; a fifth that overflowed in the same wait is consumed unnamed.
        named = re.findall(r"(\d+) entries needed, max_tile_entries = (\d+) \(forward pass (0x[0-9a-fA-F]+)\)", str(error))
        return [Overflow(int(n), int(c), int(h, 16)) for n, c, h in named]

    @classmethod
    def split(cls, error, own_handles) -> tuple:
        """``(mine, others)``: the records about ``own_handles``' passes, and whether the report also names passes of another owner."""
        own = {int(h) for h in own_handles}
        named = cls.parse(error)
        mine = [o for o in named if o.handle in own]
        return mine, len(mine) < len(named)

    @classmethod
    def passes_named(cls, error) -> set:
        return {o.handle for o in cls.parse(error)}

    def post(self, error) -> None:
        self.pending.append(error)
        del self.pending[:-self.keep]

    def take(self, own_handles) -> Optional[Exception]:
        """The oldest pending report that names one of ``own_handles`` (removed), or None."""
        own = {int(h) for h in own_handles}
        for i, e in enumerate(self.pending):
            if self.passes_named(e) & own:
                return self.pending.pop(i)
        return None


class HipDevice:
    """``GPUDevice`` + ``GPUQueue`` on one MI355X: a HIP ordinal and torch's current stream on it."""

    def __init__(self, ordinal: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("webdgs_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = _lib.load()
        self.ordinal = ordinal
        self.torch_device = torch.device("cuda", ordinal)
        torch.cuda.set_device(ordinal)
        # One explicit stream shared by torch (allocations' fills, H2D copies, RCCL hand-off) and the library's kernels.
        # torch's default stream has a NULL handle, which wdgs_device_create reads as "create your own stream" -- that
        # would leave torch.zeros() fills unordered against our kernels -- so make a real stream current instead.
        self.torch_stream = torch.cuda.Stream(self.torch_device)
        torch.cuda.set_stream(self.torch_stream)
        stream = self.torch_stream.cuda_stream
        assert stream, "torch returned a NULL stream handle"
        h = C.c_void_p()
        check(self.lib.wdgs_device_create(ordinal, C.c_void_p(stream), C.byref(h)))
        self.handle = h
        self.queue = _Queue(self)
        self.capacityReports = CapacityReports()
        self._keepalive: list = []

    def createCommandEncoder(self, label: str = "", record: bool = False) -> HipEncoder:
        return HipEncoder(self, label, record)

    def createBuffer(self, size: int, label: str = "") -> HipBuffer:
        """Zero-filled like a WebGPU buffer."""
        t = torch.zeros(max(1, (int(size) + 3) // 4), dtype=torch.int32, device=self.torch_device)
        return HipBuffer(self, t.data_ptr(), int(size), t, label)

    def bufferFrom(self, array: np.ndarray, label: str = "") -> HipBuffer:
        a = np.ascontiguousarray(array)
        if a.nbytes == 0:  # an empty point cloud still needs a valid (never dereferenced) device address
            t = torch.zeros(4, dtype=torch.uint8, device=self.torch_device)
            return HipBuffer(self, t.data_ptr(), 0, t, label)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.torch_device)
        return HipBuffer(self, t.data_ptr(), a.nbytes, t, label)

    def view(self, ptr: int, size: int, label: str = "") -> HipBuffer:
        return HipBuffer(self, ptr, size, None, label)

    def synchronize(self) -> None:
        check(self.lib.wdgs_device_synchronize(self.handle))
        self._keepalive.clear()

    def memoryInfo(self) -> dict:
        """``device.limits`` as far as memory goes (trainer.ts:147): bytes free / total on the device, and what the library's allocation cache holds."""
        f, t, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(self.lib.wdgs_device_memory_info(self.handle, C.byref(f), C.byref(t), C.byref(c)))
        return dict(free=int(f.value), total=int(t.value), cached=int(c.value))

    def selectLane(self, lane: int) -> None:
        """Directs every later encode / submit to lane 0 (this device's stream) or an internal one, 1..MAX_LANES-1 (``include/webdgs.h``: lanes)."""
        check(self.lib.wdgs_device_select_lane(self.handle, int(lane)))

    def laneMark(self, lane: int, mark: int) -> None:
        """Remembers the current end of ``lane`` in mark ``mark`` (``wdgs_device_lane_mark``) for ``laneWaitMark`` calls made later."""
        check(self.lib.wdgs_device_lane_mark(self.handle, int(lane), int(mark)))

    def laneWaitMark(self, lane: int, mark: int) -> None:
        check(self.lib.wdgs_device_lane_wait_mark(self.handle, int(lane), int(mark)))

    def laneOrder(self, waiter: int, signal: int) -> None:
        """What lane ``waiter`` gets from now on runs after what lane ``signal`` has been given so far (device-side, no host wait)."""
        check(self.lib.wdgs_device_lane_order(self.handle, int(waiter), int(signal)))

    def setProfiling(self, enabled: bool) -> None:
        check(self.lib.wdgs_device_set_profiling(self.handle, 1 if enabled else 0))

    def kernelTimes(self, reset: bool = False) -> dict:
        n = C.c_uint32(0)
        arr = (_lib.KernelTime * 128)()
        check(self.lib.wdgs_device_get_kernel_times(self.handle, arr, 128, C.byref(n)))
        out = {arr[i].name.decode(): (arr[i].launches, arr[i].total_ms) for i in range(min(n.value, 128))}
        if reset:
            check(self.lib.wdgs_device_reset_kernel_times(self.handle))
        return out

    def destroy(self) -> None:
        """Drains the stream and frees the library-side device.  Ops and command buffers should be destroyed first; one that is
        destroyed later only releases its memory (include/webdgs.h "teardown order").  Idempotent."""
        if self.handle:
            self.lib.wdgs_encoder_abort(self.handle)
            self.lib.wdgs_device_destroy(self.handle)
            self.handle = None
        self._keepalive.clear()


@dataclasses.dataclass
class PointCloud:
    """``PointCloud`` of ``src/utils/load-pointcloud.ts:16-23``."""

    type: str
    num_points: int
    sh_deg: int
    gaussian_3d_buffer: HipBuffer
    sh_buffer: HipBuffer
    # set while an Optimizer trains this cloud with deferred SH writes (``Optimizer.setDeferredSH``): the compact SH-DC array every forward pass
    # built on the cloud reads in place of the rows' first six bytes -- the trainer's passes and a Viewer's alike, without the host knowing
    dc_words: Optional[HipBuffer] = None


def createPointCloud(device: HipDevice, gaussians: np.ndarray, sh: np.ndarray, sh_deg: int) -> PointCloud:
    n = int(gaussians.shape[0])
    return PointCloud("full", n, int(sh_deg), device.bufferFrom(gaussians.astype(np.uint32, copy=False), "gaussian_3d_buffer"),
                      device.bufferFrom(sh.astype(np.uint32, copy=False), "sh_buffer"))


def allocatePointCloudLike(device: HipDevice, template: PointCloud, options: dict) -> PointCloud:
    """``allocatePointCloudLike`` (``src/utils/allocate-pointcloud.ts:8-44``)."""
    n = max(1, int(options["numPoints"]))
    tp = max(1, int(template.num_points))
    bpg = max(1, template.gaussian_3d_buffer.size // tp)
    bps = max(1, template.sh_buffer.size // tp)
    return PointCloud(template.type or "normal", n, template.sh_deg or 0, device.createBuffer(n * bpg, "resized gaussian_3d_buffer"),
                      device.createBuffer(n * bps, "resized sh_buffer"))


# ----------------------------------------------------------------------------- scanner / sorter
class PrefixScanner:
    """``PrefixScanner`` (``src/prefix/prefix.ts:26-43``)."""

    def __init__(self, max_elements: int, device: HipDevice):
        self.device, self.max_elements = device, int(max_elements)
        h = C.c_void_p()
        check(device.lib.wdgs_prefix_scanner_create(device.handle, self.max_elements, C.byref(h)))
        self.handle = h
        self.input_buffer = device.view(device.lib.wdgs_prefix_scanner_input(h), 4 * self.max_elements, "prefix-input")
        self.output_buffer = device.view(device.lib.wdgs_prefix_scanner_output(h), 4 * self.max_elements, "prefix-output")

    def set_count(self, count: int) -> dict:
        check(self.device.lib.wdgs_prefix_scanner_set_count(self.handle, int(count)))
        return {"num_workgroups": (int(count) + 4095) // 4096}

    def scan(self, encoder: Optional[HipEncoder] = None) -> None:
        check(self.device.lib.wdgs_prefix_scanner_scan(self.handle))

    def destroy(self) -> None:
        if self.handle:
            self.device.lib.wdgs_prefix_scanner_destroy(self.handle)
            self.handle = None


def get_prefix_scanner(max_elements: int, device: HipDevice) -> PrefixScanner:
    return PrefixScanner(max_elements, device)


class DynamicSortStuff:
    """``DynamicSortStuff`` (``src/sort/sort_dynamic.ts:9-24``): count comes from ``stats_buffer[0]`` on the device."""

    def __init__(self, max_capacity: int, device: HipDevice, stats_buffer: HipBuffer):
        self.device = device
        h = C.c_void_p()
        check(device.lib.wdgs_sorter_create(device.handle, int(max_capacity), C.c_void_p(stats_buffer.ptr), C.byref(h)))
        self.handle = h
        cap = device.lib.wdgs_sorter_capacity(h)
        self.capacity = cap
        self.ping_pong = [dict(sort_depths_buffer=device.view(device.lib.wdgs_sorter_keys(h, i), 4 * cap),
                               sort_indices_buffer=device.view(device.lib.wdgs_sorter_values(h, i), 4 * cap)) for i in range(2)]
        self.final_out_index = 0

    def sort(self, encoder: Optional[HipEncoder] = None, key_bits: int = 32) -> None:
        check(self.device.lib.wdgs_sorter_sort(self.handle, int(key_bits)))
        self.final_out_index = self.device.lib.wdgs_sorter_final_out_index(self.handle)

    def destroy(self) -> None:
        if self.handle:
            self.device.lib.wdgs_sorter_destroy(self.handle)
            self.handle = None


def get_dynamic_sorter(max_capacity: int, device: HipDevice, stats_buffer: HipBuffer) -> DynamicSortStuff:
    return DynamicSortStuff(max_capacity, device, stats_buffer)


# ----------------------------------------------------------------------------- TiledForwardPass
class TiledForwardPass:
    """``TiledForwardPass`` (``src/renderers/tiled-forward-pass.ts:62-534``)."""

    def __init__(self, device: HipDevice, pointCloud: PointCloud, cameraBuffer: HipBuffer, config: dict):
        self.device, self.pointCloud, self.cameraBuffer = device, pointCloud, cameraBuffer
        self.destroyed = False
        cfg = _lib.TiledForwardConfig(
            num_points=pointCloud.num_points, sh_deg=pointCloud.sh_deg, viewport_width=int(config["viewportWidth"]),
            viewport_height=int(config["viewportHeight"]), gaussian_scale=float(config.get("gaussianScale", 1.0)),
            point_size_px=float(config.get("pointSizePx", 3.0)), max_splat_radius_px=float(config.get("maxSplatRadiusPx", 128.0)),
            render_mode=1 if config.get("renderMode", "gaussian") == "gaussian" else 0,
            max_tile_entries=int(config.get("maxTileEntries", 0)), compat_caps=1 if config.get("compatCaps", False) else 0)
        h = C.c_void_p()
        check(device.lib.wdgs_tiled_forward_create(device.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        self._dc_source: Optional[HipBuffer] = None

    def syncDcSource(self) -> None:
        """Follows the cloud's ``dc_words`` (set by ``Optimizer.setDeferredSH``): a pass built on a cloud that is being trained renders the
        trained colours even if its host never heard of deferred SH writes (the reference's Viewer shares the Trainer's PointCloud,
        main.ts:389, 524)."""
        want = getattr(self.pointCloud, "dc_words", None)
        if want is not getattr(self, "_dc_source", None):
            self.setDcSource(want)

    def encode(self, encoder: Optional[HipEncoder] = None, options: Optional[dict] = None) -> None:
        skip = 1 if (options or {}).get("skipSort") else 0
        self.syncDcSource()
        check(self.device.lib.wdgs_tiled_forward_encode(self.handle, self.pointCloud.gaussian_3d_buffer.ptr, self.pointCloud.sh_buffer.ptr,
                                                        self.cameraBuffer.ptr, skip))

    def encodeProjected(self, encoder: Optional["HipEncoder"] = None) -> None:
        """The rest of ``encode`` (scan, emit, sort) for a pass whose K1 ran through ``projectViews`` (view-batched step; no reference
        counterpart)."""
        check(self.device.lib.wdgs_tiled_forward_encode_projected(self.handle))

    def isProjected(self) -> bool:
        """True while the pass holds a projection (``projectViews``) that no ``encode*`` call made through this host has consumed or
        overwritten since (the rest of the pass can run once per projection)."""
        return bool(self.device.lib.wdgs_tiled_forward_is_projected(self.handle))

    def setCameraBuffer(self, buffer: HipBuffer) -> None:
        self.cameraBuffer = buffer

    def setDcSource(self, dcWords: Optional[HipBuffer]) -> None:
        """K1 takes the SH-DC halves from the optimizer's compact array (``Optimizer.setDeferredSH``) instead of the cloud's rows; ``None``
        restores the rows.  No reference counterpart (include/webdgs.h)."""
        self._dc_source = dcWords  # (kept alive)
        check(self.device.lib.wdgs_tiled_forward_set_dc_source(self.handle, dcWords.ptr if dcWords is not None else None))

    def setPointCloud(self, pointCloud: PointCloud) -> bool:
        """Adopts a point cloud of another size (``wdgs_tiled_forward_resize``: buffers reused, or re-allocated with headroom) instead of
        the destroy + construct of ``applyPointCloudSwap`` (trainer.ts:201-237).  False -- nothing changed -- if the SH degree differs."""
        if pointCloud.sh_deg != self.pointCloud.sh_deg:
            return False
        check(self.device.lib.wdgs_tiled_forward_resize(self.handle, pointCloud.num_points))
        self.pointCloud = pointCloud
        return True

    def setGaussianScale(self, value: float) -> None:
        check(self.device.lib.wdgs_tiled_forward_set_gaussian_scale(self.handle, float(value)))

    def setPointSize(self, value: float) -> None:
        check(self.device.lib.wdgs_tiled_forward_set_point_size(self.handle, float(value)))

    def setRenderMode(self, mode: str) -> None:
        check(self.device.lib.wdgs_tiled_forward_set_render_mode(self.handle, 1 if mode == "gaussian" else 0))

    def setViewport(self, width: int, height: int) -> None:
        check(self.device.lib.wdgs_tiled_forward_set_viewport(self.handle, int(width), int(height)))

    def _res(self) -> _lib.TiledForwardResources:
        r = _lib.TiledForwardResources()
        check(self.device.lib.wdgs_tiled_forward_get_resources(self.handle, C.byref(r)))
        return r

    def getResources(self) -> dict:
        r, d, n = self._res(), self.device, max(1, self.pointCloud.num_points)
        return dict(splatBuffer=d.view(r.splat_buffer, 24 * n), depthsBuffer=d.view(r.depths_buffer, 4 * n),
                    tileKeysBuffer=d.view(r.tile_keys_buffer, 4 * r.max_tile_entries), tileIndicesBuffer=d.view(r.tile_indices_buffer, 4 * r.max_tile_entries),
                    tileOffsetsBuffer=d.view(r.tile_offsets_buffer, 4 * n), tileCountsBuffer=d.view(r.tile_counts_buffer, 4 * n),
                    statsBuffer=d.view(r.stats_buffer, 16), numTilesX=r.num_tiles_x, numTilesY=r.num_tiles_y, totalTiles=r.total_tiles,
                    maxTileEntries=r.max_tile_entries, settings=np.array(list(r.settings), np.float32))

    def getSortedIndicesBuffer(self) -> HipBuffer:
        return self.getResources()["tileIndicesBuffer"]

    def getSortedKeysBuffer(self) -> HipBuffer:
        return self.getResources()["tileKeysBuffer"]

    def getTileOffsetsBuffer(self) -> HipBuffer:
        return self.getResources()["tileOffsetsBuffer"]

    def getStatsBuffer(self) -> HipBuffer:
        return self.getResources()["statsBuffer"]

    def check(self) -> np.ndarray:
        """Synchronises; raises ``CapacityError`` if the last encode overflowed ``maxTileEntries``. Returns the 4 stats words."""
        st = (C.c_uint32 * 4)()
        check(self.device.lib.wdgs_tiled_forward_check(self.handle, st))
        return np.array(list(st), np.uint32)

    def setLongLists(self, threshold: int, maxItems: int = 0, maxRows: int = 0) -> None:
        """Long tile lists (``include/webdgs.h``: wdgs_tiled_forward_set_long_lists): tiles with more than ``threshold`` entries get per-pixel lists
        (0: off); ``maxItems`` / ``maxRows`` size the work (0: keep).  Synchronises; drop command buffers recorded against the pass."""
        check(self.device.lib.wdgs_tiled_forward_set_long_lists(self.handle, int(threshold), int(maxItems), int(maxRows)))

    def longListStats(self) -> dict:
        """The last frame's long-list work: what it wanted and what the pass has room for (synchronises)."""
        st = (C.c_uint32 * 12)()
        check(self.device.lib.wdgs_tiled_forward_long_list_stats(self.handle, st))
        keys = ("blocksWanted", "itemsWanted", "forwardQueue", "backwardQueue", "rowsUsed", "rowsWanted", "stalled", "_", "maxItems", "maxBlocks", "maxRows", "threshold")
        return {k: int(v) for k, v in zip(keys, st) if k != "_"}

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_tiled_forward_destroy(self.handle)
        self.handle = None


# ----------------------------------------------------------------------------- TiledRasterizer
DEPTH_KINDS = {"expected": 1, "median": 2, "weight_sum": 4}  # WDGS_DEPTH_* (include/webdgs.h)


def _depth_mask(kinds) -> int:
    mask = 0
    for k in ((kinds,) if isinstance(kinds, str) else kinds):
        if k not in DEPTH_KINDS:
            raise ValueError(f"unknown depth kind {k!r}: one of {sorted(DEPTH_KINDS)}")
        mask |= DEPTH_KINDS[k]
    return mask


class TiledRasterizer:
    """``TiledRasterizer`` (``src/renderers/tiled-rasterizer.ts:34-368``) without the swap-chain blit."""

    def __init__(self, config: dict):
        self.device: HipDevice = config["device"]
        self.forwardPass: TiledForwardPass = config["forwardPass"]
        self.destroyed = False
        self.width = self.height = 0
        h = C.c_void_p()
        check(self.device.lib.wdgs_tiled_rasterizer_create(self.device.handle, self.forwardPass.handle, 1 if config.get("compatCaps") else 0, C.byref(h)))
        self.handle = h

    def encode(self, encoder: Optional[HipEncoder], width: int, height: int) -> None:
        check(self.device.lib.wdgs_tiled_rasterizer_encode(self.handle, int(width), int(height)))
        self.width, self.height = int(width), int(height)

    def _get(self, fn, nbytes: int) -> HipBuffer:
        p = C.c_void_p()
        check(fn(self.handle, C.byref(p)))
        return self.device.view(p.value, nbytes)

    def getOutputTextureView(self) -> HipBuffer:
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_output, 4 * self.width * self.height)

    def getAlphaTextureView(self) -> HipBuffer:
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_alpha, 4 * self.width * self.height)

    def getNContribTextureView(self) -> HipBuffer:
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_n_contrib, 4 * self.width * self.height)

    def getTileOffsetsBuffer(self) -> HipBuffer:
        tiles = ((self.width + 15) // 16) * ((self.height + 15) // 16)
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_tile_offsets, 4 * (tiles + 1))

    def encodeDepth(self, encoder: Optional[HipEncoder], kinds=("expected",)) -> None:
        """Depth images of the frame the last ``encode`` rasterized (no reference counterpart): ``kinds`` is a sequence of
        ``DEPTH_KINDS`` names or the bit mask itself.  The first use of a kind allocates its image and cannot be recorded."""
        mask = int(kinds) if isinstance(kinds, (int, np.integer)) else _depth_mask(kinds)
        check(self.device.lib.wdgs_tiled_rasterizer_encode_depth(self.handle, mask))

    def getDepthTextureView(self, kind: str = "expected") -> HipBuffer:
        """f32[W*H] of one kind the last ``encodeDepth`` wrote; raises ``StateError`` otherwise."""
        p = C.c_void_p()
        check(self.device.lib.wdgs_tiled_rasterizer_get_depth(self.handle, _depth_mask((kind,)), C.byref(p)))
        return self.device.view(p.value, 4 * self.width * self.height)

    def encodeContribution(self, encoder: Optional[HipEncoder], statsBuffer: HipBuffer) -> None:
        """Adds the per-Gaussian contribution of the frame the last ``encode`` rasterized into ``statsBuffer`` (``createContributionBuffer``; DESIGN.md
        section 11; no reference counterpart).  Allocates nothing, so it records."""
        n = self.forwardPass.pointCloud.num_points
        if statsBuffer.size < CONTRIBUTION_RECORD_BYTES * n:
            raise ValueError(f"encodeContribution: the statistics buffer holds {statsBuffer.size} bytes, {n} Gaussians need {CONTRIBUTION_RECORD_BYTES * n}")
        check(self.device.lib.wdgs_tiled_rasterizer_encode_contribution(self.handle, statsBuffer.ptr))

    def encodeNormal(self, encoder: Optional[HipEncoder]) -> None:
        """The normal map of the frame the last ``encode`` rasterized (no reference counterpart): one packed view-space normal
        per Gaussian of the forward pass's cloud under its camera, composited with the colour image's weights.  The first use, and the first after
        the point count or the size changed, allocates and cannot be recorded."""
        f = self.forwardPass
        check(self.device.lib.wdgs_tiled_rasterizer_encode_normal(self.handle, f.pointCloud.gaussian_3d_buffer.ptr, f.cameraBuffer.ptr))

    def getNormalTextureView(self) -> HipBuffer:
        """rgba32f[W*H] ``{N.x, N.y, N.z, A}`` of the last ``encodeNormal`` (``N`` un-normalised: ``|N| <= A``); raises ``StateError`` before it."""
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_normal, 16 * self.width * self.height)

    def getGaussianNormals(self) -> HipBuffer:
        """u32[numPoints]: the packed per-Gaussian normals of the last ``encodeNormal`` (``decodeNormals``); raises ``StateError`` before it."""
        return self._get(self.device.lib.wdgs_tiled_rasterizer_get_gaussian_normals, 4 * max(1, self.forwardPass.pointCloud.num_points))

    def blitToTexture(self, encoder: Optional[HipEncoder], target: HipBuffer, width: Optional[int] = None, height: Optional[int] = None) -> None:
        """``blitToTexture(encoder, targetView)`` (tiled-rasterizer.ts:333-357): ``target`` is an rgba8 image buffer of
        ``width x height`` (default: the rasterizer's own size); raises before the first ``encode`` like the reference."""
        w, h = int(width or self.width), int(height or self.height)
        if self.handle is not None and w * h * 4 > target.size:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"blitToTexture: target of {target.size} bytes is smaller than {w}x{h} rgba8")
        check(self.device.lib.wdgs_tiled_rasterizer_blit(self.handle, target.ptr, max(w, 0), max(h, 0)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_tiled_rasterizer_destroy(self.handle)
        self.handle = None


# ----------------------------------------------------------------------------- TiledBackwardPass
def _training_config(tc: Optional[dict]) -> _lib.TrainingConfig:
    tc = tc or {}
    return _lib.TrainingConfig(float(tc.get("lambda_l1", 0.8)), float(tc.get("lambda_l2", 0.0)), float(tc.get("lambda_dssim", 0.2)),
                               float(tc.get("c1", 0.01 * 0.01)), float(tc.get("c2", 0.03 * 0.03)))


# trainingConfig["dssim_mode"] -> WDGS_DSSIM_* (include/webdgs.h): the loss the backward pass differentiates
DSSIM_MODES = {"reference": 0, "gaussian": 1}


def dssim_mode(tc: Optional[dict]) -> int:
    """The ``WDGS_DSSIM_*`` value of a training config's ``dssim_mode``: ``"reference"`` (the default; the reference's heuristic gradient) or
    ``"gaussian"`` (the exact gradient of the 3DGS loss with the 11x11 Gaussian-window SSIM).  ValueError otherwise."""
    mode = (tc or {}).get("dssim_mode")
    mode = "reference" if mode is None else mode
    if not isinstance(mode, str) or mode not in DSSIM_MODES:
        raise ValueError(f"dssim_mode must be one of {sorted(DSSIM_MODES)}, not {mode!r}")
    return DSSIM_MODES[mode]


class TiledBackwardPass:
    """``TiledBackwardPass`` (``src/renderers/tiled-backward-pass.ts:71-861``).  ``trainingConfig["dssim_mode"]`` (no reference counterpart)
    chooses the loss: ``"reference"`` (default) or ``"gaussian"``; see ``dssim_mode``."""

    def __init__(self, device: HipDevice, pointCloud: PointCloud, config: dict):
        mode = dssim_mode(config.get("trainingConfig"))
        self.device, self.pointCloud = device, pointCloud
        self.destroyed = False
        self.viewportWidth, self.viewportHeight = int(config["viewportWidth"]), int(config["viewportHeight"])
        self.trainingConfig = dict(config.get("trainingConfig") or {})
        cfg = _lib.TiledBackwardConfig(pointCloud.num_points, pointCloud.sh_deg, self.viewportWidth, self.viewportHeight, _training_config(self.trainingConfig),
                                       float(config.get("gaussianScale", 1.0)), float(config.get("pointSizePx", 3.0)),
                                       float(config.get("maxSplatRadiusPx", 128.0)))
        h = C.c_void_p()
        check(device.lib.wdgs_tiled_backward_create(device.handle, C.byref(cfg), C.byref(h)))
        self.handle = h
        if mode:
            check(device.lib.wdgs_tiled_backward_set_dssim_mode(h, mode))

    @staticmethod
    def _resources(res: dict) -> _lib.TiledBackwardResources:
        def p(k):
            b = res.get(k)
            return b.ptr if b is not None else None
        return _lib.TiledBackwardResources(p("splatBuffer"), p("tileOffsetsBuffer"), p("tileIndicesBuffer"), p("cameraBuffer"), p("alphaTexture"),
                                           p("nContribTexture"))

    def setPointCloud(self, pointCloud: PointCloud) -> bool:
        """See ``TiledForwardPass.setPointCloud`` (``wdgs_tiled_backward_resize``)."""
        if pointCloud.sh_deg != self.pointCloud.sh_deg:
            return False
        check(self.device.lib.wdgs_tiled_backward_resize(self.handle, pointCloud.num_points))
        self.pointCloud = pointCloud
        return True

    def encode(self, encoder: Optional[HipEncoder], predictedTexture: HipBuffer, targetTexture: HipBuffer, forwardResources: dict, options=None) -> None:
        r = self._resources(forwardResources)
        check(self.device.lib.wdgs_tiled_backward_encode(self.handle, predictedTexture.ptr, targetTexture.ptr, C.byref(r), self.pointCloud.gaussian_3d_buffer.ptr))

    def encodeRaster(self, encoder: Optional[HipEncoder], predictedTexture: HipBuffer, targetTexture: HipBuffer, forwardResources: dict) -> None:
        """First half of ``encode`` (K15 loss gradient, clear, K16 backward raster): ``wdgs_tiled_backward_encode_raster``."""
        r = self._resources(forwardResources)
        check(self.device.lib.wdgs_tiled_backward_encode_raster(self.handle, predictedTexture.ptr, targetTexture.ptr, C.byref(r)))

    def encodeGeometry(self, encoder: Optional[HipEncoder], cameraBuffer: HipBuffer, accumulate: Optional[dict] = None) -> None:
        """Second half of ``encode`` (K17).  ``accumulate`` (a batched step): ``dict(sums, visible, tileCounts, guard, stats, first)`` --
        K17 then also adds this view's gradient to the step's fp32 block and folds the forward pass's overflow word (``stats`` + 8
        bytes) into the guard word, instead of ``storeGradients`` / ``accumulateGradients`` + ``guardAccumulate`` afterwards."""
        into = None
        if accumulate is not None:
            a = accumulate
            into = C.byref(_lib.ViewAccumulate(a["sums"].ptr, a["visible"].ptr, a["tileCounts"].ptr, a["guard"].ptr, a["stats"].ptr + 8, 1 if a["first"] else 0))
        check(self.device.lib.wdgs_tiled_backward_encode_geometry(self.handle, cameraBuffer.ptr, self.pointCloud.gaussian_3d_buffer.ptr, into))

    def computeLossOnly(self, encoder, predictedTexture: HipBuffer, targetTexture: HipBuffer) -> None:
        check(self.device.lib.wdgs_tiled_backward_compute_loss_only(self.handle, predictedTexture.ptr, targetTexture.ptr))

    def computeMetricMap(self, encoder, predictedTexture: HipBuffer, targetTexture: HipBuffer, options: Optional[dict] = None) -> None:
        thr = float((options or {}).get("threshold", 0.5))
        check(self.device.lib.wdgs_tiled_backward_compute_metric_map(self.handle, predictedTexture.ptr, targetTexture.ptr, thr))

    def computeMetricCounts(self, encoder, resources: dict, options: Optional[dict] = None) -> None:
        r = self._resources(resources)
        clear = 1 if (options or {}).get("clear", True) else 0
        n_inst = resources["tileIndicesBuffer"].size // 4
        check(self.device.lib.wdgs_tiled_backward_compute_metric_counts(self.handle, C.byref(r), n_inst, clear))

    def normalizeMetricCounts(self, encoder, options: dict) -> None:
        check(self.device.lib.wdgs_tiled_backward_normalize_metric_counts(self.handle, max(1, int(options["divisor"]))))

    def setViewport(self, width: int, height: int) -> None:
        check(self.device.lib.wdgs_tiled_backward_set_viewport(self.handle, int(width), int(height)))
        self.viewportWidth, self.viewportHeight = int(width), int(height)

    def setTrainingConfig(self, next_cfg: dict) -> None:
        merged = dict(self.trainingConfig, **{k: v for k, v in next_cfg.items() if v is not None})
        mode = dssim_mode(merged)
        self.trainingConfig = merged
        tc = _training_config(self.trainingConfig)
        check(self.device.lib.wdgs_tiled_backward_set_training_config(self.handle, C.byref(tc)))
        check(self.device.lib.wdgs_tiled_backward_set_dssim_mode(self.handle, mode))

    def setGradientOutput(self, enabled: bool) -> None:
        """Whether ``Optimizer.stepWithGeometry`` also writes K17's packed gradient to ``getGradientsBuffer()`` (default: yes, as the
        reference's K17 does).  A host that never reads it saves 32 bytes per Gaussian and step; ``encode`` / ``encodeGeometry`` always write it."""
        check(self.device.lib.wdgs_tiled_backward_set_gradient_output(self.handle, 1 if enabled else 0))

    def getGradientsBuffer(self) -> HipBuffer:
        return self.device.view(self.device.lib.wdgs_tiled_backward_gradients(self.handle), 32 * max(1, self.pointCloud.num_points))

    def setMetricCountsTarget(self, counts: Optional[HipBuffer]) -> None:
        """``computeMetricCounts`` of this pass adds into ``counts`` (another pass's ``getMetricCountsBuffer()``) instead of its own array;
        ``None`` restores its own.  Lets several passes take the metric views of one densify event on different lanes (integer atomics:
        any order gives the same bits).  No reference counterpart."""
        self._metric_target = counts  # (kept alive)
        check(self.device.lib.wdgs_tiled_backward_set_metric_counts_target(self.handle, counts.ptr if counts is not None else None))

    def getMetricCountsBuffer(self) -> HipBuffer:
        return self.device.view(self.device.lib.wdgs_tiled_backward_metric_counts(self.handle), 4 * max(1, self.pointCloud.num_points))

    def getLossTextureView(self) -> HipBuffer:
        return self.device.view(self.device.lib.wdgs_tiled_backward_loss_image(self.handle), 16 * self.viewportWidth * self.viewportHeight)

    def getMetricMapTextureView(self) -> HipBuffer:
        return self.device.view(self.device.lib.wdgs_tiled_backward_metric_map(self.handle), 4 * self.viewportWidth * self.viewportHeight)

    def getMetricMapTexture(self) -> HipBuffer:
        """``getMetricMapTexture`` (tiled-backward-pass.ts): texture and view are the same r32uint image buffer here."""
        return self.getMetricMapTextureView()

    def getAccumulatorsBuffer(self) -> HipBuffer:
        """INTERNAL (parity tests): i32[N*12] fixed-point accumulators of the last encode."""
        return self.device.view(self.device.lib.wdgs_tiled_backward_accumulators(self.handle), 48 * max(1, self.pointCloud.num_points))

    def getMetricMinMaxBuffer(self) -> HipBuffer:
        return self.device.view(self.device.lib.wdgs_tiled_backward_metric_minmax(self.handle), 8)

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_tiled_backward_destroy(self.handle)
        self.handle = None


def downsampleRGBA8(device: HipDevice, src: HipBuffer, src_w: int, src_h: int, dst: HipBuffer, dst_w: int, dst_h: int) -> None:
    """The GT down-sample render pass of ``trainer.ts:303-328`` (``blit.wgsl`` ``fs_main`` with a linear sampler)."""
    check(device.lib.wdgs_downsample_rgba8(device.handle, src.ptr, src_w, src_h, dst.ptr, dst_w, dst_h))


def depthToRGBA8(device: HipDevice, depth: HipBuffer, width: int, height: int, near: float, far: float, target: HipBuffer) -> None:
    """A depth image (f32, ``getDepthTextureView``) as rgba8 for presentation: inverse depth between ``near`` (white) and ``far`` (black), depth 0
    black, alpha 255 (``wdgs_depth_to_rgba8``).  Stream-ordered; no reference counterpart."""
    n = int(width) * int(height)
    if depth.size < 4 * n or target.size < 4 * n:
        raise ValueError(f"depthToRGBA8: buffers too small for {width}x{height}")
    check(device.lib.wdgs_depth_to_rgba8(device.handle, depth.ptr, int(width), int(height), float(near), float(far), target.ptr))


# ----------------------------------------------------------------------------- normal maps (no reference counterpart)
NO_NORMAL = 0x80008000  # the packed word of a Gaussian without a normal


def decodeNormals(words) -> np.ndarray:
    """Packed per-Gaussian normals (``getGaussianNormals``) as float32 ``[n, 3]`` unit vectors, by the decode of DESIGN.md section 12, operation by
    operation in float32 as the compositing kernel evaluates it; ``NO_NORMAL`` gives the zero vector.  Host side (numpy)."""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    one, q = np.float32(1), np.float32(32767)
    u = (w & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.float32) / q
    v = (w >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(np.float32) / q
    au, av = np.abs(u), np.abs(v)
    t = (one - au) - av
    fold = t < 0
    x = np.where(fold, np.copysign(one - av, u), u)
    y = np.where(fold, np.copysign(one - au, v), v)
    z = -t
    length = np.sqrt((x * x + y * y) + z * z)
    out = np.stack([x / length, y / length, z / length], axis=1).astype(np.float32)
    out[w == np.uint32(NO_NORMAL)] = 0
    return out


def depthToNormals(device: HipDevice, depth: HipBuffer, width: int, height: int, camera, target: HipBuffer) -> None:
    """The normals of an f32 depth image (``getDepthTextureView``, or any other) by central differences of its back-projection
    (``loaders.backprojectDepth``'s convention): rgba32f ``{n, 1}`` into ``target``, all zero where a neighbour is missing
    (``wdgs_depth_to_normals``).  ``camera``: the 68-float block, or the pair ``(proj[0][0], proj[1][1])``.  Stream-ordered."""
    n = int(width) * int(height)
    if depth.size < 4 * n or target.size < 16 * n:
        raise ValueError(f"depthToNormals: buffers too small for {width}x{height}")
    c = np.asarray(camera, np.float32).reshape(-1)
    p00, p11 = (c[32], c[37]) if c.size == 68 else (c[0], c[1])
    check(device.lib.wdgs_depth_to_normals(device.handle, depth.ptr, int(width), int(height), float(p00), float(p11), target.ptr))


def encodeNormalAgreement(device: HipDevice, normal: HipBuffer, depthNormals: HipBuffer, width: int, height: int, out: HipBuffer) -> None:
    """Stream-ordered ``normalAgreement``: the three u64 sums into the first 24 bytes of ``out``.  No host wait."""
    n = int(width) * int(height)
    if normal.size < 16 * n or depthNormals.size < 16 * n or out.size < 24:
        raise ValueError(f"normalAgreement: buffers too small for {width}x{height}")
    check(device.lib.wdgs_normal_agreement(device.handle, normal.ptr, depthNormals.ptr, int(width), int(height), out.ptr))


def normalAgreement(device: HipDevice, normal: HipBuffer, depthNormals: HipBuffer, width: int, height: int) -> dict:
    """How well a composited normal image (``getNormalTextureView``) agrees with a depth-normal image (``depthToNormals``), over the pixels with
    ``A >= 0.5``, ``|N| > 0`` and a valid depth normal: the exact integer sums ``sum_e`` (of ``rint(A (1 - cos) 2^24)``) and ``sum_a`` (of
    ``rint(A 2^24)``), ``pixels``, and ``value = sum_e / sum_a``, the weight-averaged ``1 - cos`` (nan when nothing counts).  Synchronises."""
    out = device.createBuffer(24, "normal agreement")
    try:
        encodeNormalAgreement(device, normal, depthNormals, width, height, out)
        e, a, cnt = (int(x) for x in out.read(np.uint64, count=3))
    finally:
        out.destroy()
    return dict(sum_e=e, sum_a=a, pixels=cnt, value=(e / a) if a else float("nan"))


def normalToRGBA8(device: HipDevice, normal: HipBuffer, width: int, height: int, target: HipBuffer) -> None:
    """A normal image as rgba8 for presentation: ``round(255 (0.5 + 0.5 (n_x, -n_y, -n_z)))`` of the normalised normal (facing the camera: blue), black
    where ``|N| = 0``, alpha 255 (``wdgs_normal_to_rgba8``).  Stream-ordered."""
    n = int(width) * int(height)
    if normal.size < 16 * n or target.size < 4 * n:
        raise ValueError(f"normalToRGBA8: buffers too small for {width}x{height}")
    check(device.lib.wdgs_normal_to_rgba8(device.handle, normal.ptr, int(width), int(height), target.ptr))


# ----------------------------------------------------------------------------- TSDF fusion and mesh extraction (no reference counterpart)
class TSDFVolume:
    """A device TSDF volume (``wdgs_tsdf_volume``): an axis-aligned grid of ``dims = (nx, ny, nz)`` voxels of ``voxelSize`` in world space, x fastest,
    voxel ``(i, j, k)`` centred at ``origin + (i + .5, j + .5, k + .5) voxelSize``.  ``integrate`` fuses one depth image per call, ``extractTriangles`` /
    ``extractMesh`` take the zero level set as triangles by marching tetrahedra.  ``truncation=None``: 4 voxels."""

    def __init__(self, device: HipDevice, origin, voxelSize: float, dims, truncation: Optional[float] = None, maxWeight: float = 64.0, colour: bool = True):
        self.device = device
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self.voxelSize = float(np.float32(voxelSize))
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3:
            raise ValueError("TSDFVolume: dims must be (nx, ny, nz)")
        self.truncation = float(np.float32(4.0 * voxelSize if truncation is None else truncation))
        self.maxWeight = float(maxWeight)
        self.colour = bool(colour)
        self.numVoxels = self.dims[0] * self.dims[1] * self.dims[2]
        self.destroyed = False
        h = C.c_void_p()
        o = (C.c_float * 3)(*[float(x) for x in self.origin])
        for d in self.dims:
            if not 0 <= d < 2 ** 32:
                raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"TSDFVolume: bad dimensions {self.dims}")
        check(device.lib.wdgs_tsdf_volume_create(device.handle, o, self.voxelSize, self.dims[0], self.dims[1], self.dims[2], self.truncation, self.maxWeight,
                                                 1 if self.colour else 0, C.byref(h)))
        self.handle = h

    @classmethod
    def fromBounds(cls, device: HipDevice, lo, hi, voxelSize: float, **kwargs) -> "TSDFVolume":
        """The volume that covers the box ``[lo, hi]`` with voxels of ``voxelSize``: origin ``lo``, dimensions rounded up (at least 2)."""
        lo64, hi64 = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        if not (np.all(np.isfinite(lo64)) and np.all(np.isfinite(hi64)) and np.all(hi64 > lo64) and voxelSize > 0):
            raise ValueError("TSDFVolume.fromBounds: needs finite lo < hi and a positive voxel size")
        dims = [max(2, int(math.ceil(float(e) / float(voxelSize)))) for e in (hi64 - lo64)]
        return cls(device, lo64, voxelSize, dims, **kwargs)

    def _get(self, fn, nbytes: int) -> HipBuffer:
        p = C.c_void_p()
        check(fn(self.handle, C.byref(p)))
        return self.device.view(p.value, nbytes)

    def getTSDFBuffer(self) -> HipBuffer:
        """f32[nz][ny][nx].  Handing it out counts as a write of the volume: ``extractTriangles`` counts anew after it."""
        return self._get(self.device.lib.wdgs_tsdf_volume_get_tsdf, 4 * self.numVoxels)

    def getWeightBuffer(self) -> HipBuffer:
        """f32[nz][ny][nx]."""
        return self._get(self.device.lib.wdgs_tsdf_volume_get_weight, 4 * self.numVoxels)

    def getColourBuffer(self) -> HipBuffer:
        """f32[3][nz][ny][nx]: the r, g and b planes; raises ``StateError`` for a volume without colour."""
        return self._get(self.device.lib.wdgs_tsdf_volume_get_rgb, 12 * self.numVoxels)

    def reset(self) -> None:
        """tsdf = 1, weight = 0, colour = 0.  Stream-ordered."""
        check(self.device.lib.wdgs_tsdf_volume_reset(self.handle))

    def integrate(self, depth: HipBuffer, camera: HipBuffer, width: int, height: int, weightSum: Optional[HipBuffer] = None, colour: Optional[HipBuffer] = None,
                  minWeightSum: float = 0.5) -> None:
        """Fuses one view: ``depth`` f32[H*W] (``getDepthTextureView``), ``camera`` the 68-float block on the device, ``weightSum`` (optional) the
        weight-sum image whose pixels below ``minWeightSum`` are ignored, ``colour`` (optional) an rgba8 image.  One pass over the volume, no atomics:
        the result depends only on the order of the calls.  Allocates nothing, so it records; an eager call waits once (it checks the block's size)."""
        n = int(width) * int(height)
        if depth.size < 4 * n or (weightSum is not None and weightSum.size < 4 * n) or (colour is not None and colour.size < 4 * n) or camera.size < 272:
            raise ValueError(f"TSDFVolume.integrate: buffers too small for {width}x{height}")
        check(self.device.lib.wdgs_tsdf_volume_integrate(self.handle, depth.ptr, weightSum.ptr if weightSum is not None else None,
                                                         colour.ptr if colour is not None else None, int(width), int(height), camera.ptr, float(minWeightSum)))

    def countTriangles(self, minWeight: float = 1.0) -> int:
        """Counts the mesh's triangles over the cells whose eight corners have ``weight >= minWeight`` (count, scan; waits)."""
        n = C.c_uint32(0)
        check(self.device.lib.wdgs_tsdf_volume_count_triangles(self.handle, float(minWeight), C.byref(n)))
        return int(n.value)

    def extractTriangles(self, minWeight: float = 1.0) -> dict:
        """The raw device output as numpy: ``dict(positions f32[F,3,3], keys u64[F,3], colours u8[F,3,4] | None)``, triangles in cell, tetrahedron
        and case order, wound counter-clockwise seen from outside."""
        total = self.countTriangles(minWeight)
        pos = self.device.createBuffer(36 * max(total, 1), "tsdf triangle positions")
        keys = self.device.createBuffer(24 * max(total, 1), "tsdf triangle keys")
        cols = self.device.createBuffer(12 * max(total, 1), "tsdf triangle colours") if self.colour else None
        try:
            check(self.device.lib.wdgs_tsdf_volume_emit_triangles(self.handle, pos.ptr, keys.ptr, cols.ptr if cols is not None else None, total))
            return dict(positions=pos.read(np.float32, count=9 * total).reshape(total, 3, 3), keys=keys.read(np.uint64, count=3 * total).reshape(total, 3),
                        colours=cols.read(np.uint8, count=12 * total).reshape(total, 3, 4) if cols is not None else None)
        finally:
            pos.destroy()
            keys.destroy()
            if cols is not None:
                cols.destroy()

    def extractTriangleBuffers(self, minWeight: float = 1.0) -> dict:
        """``extractTriangles`` without the read-back: ``dict(positions, keys, colours | None, numTriangles)``, the three as ``HipBuffer`` the caller
        destroys (f32[F][3][3], u64[F][3], rgba8[F][3]): what ``weldTrianglesDevice`` takes."""
        total = self.countTriangles(minWeight)
        pos = self.device.createBuffer(36 * max(total, 1), "tsdf triangle positions")
        keys = self.device.createBuffer(24 * max(total, 1), "tsdf triangle keys")
        cols = self.device.createBuffer(12 * max(total, 1), "tsdf triangle colours") if self.colour else None
        out = dict(positions=pos, keys=keys, colours=cols, numTriangles=total)
        try:
            check(self.device.lib.wdgs_tsdf_volume_emit_triangles(self.handle, pos.ptr, keys.ptr, cols.ptr if cols is not None else None, total))
        except BaseException:
            destroyBuffers(out)
            raise
        return out

    def extractMesh(self, minWeight: float = 1.0, weld: str = "host", simplify: Optional[float] = None, smooth: Optional[int] = None, normals: bool = False) -> dict:
        """The welded mesh: ``dict(vertices f32[V,3], faces u32[F,3], colours u8[V,3] | None, keys u64[V])``.  Vertices are the triangles' distinct edge
        keys in ascending order (equal keys carry equal position bits); triangles are kept as emitted, zero-area ones included.  ``weld="host"``: the
        triangles are read back and welded by ``weldTriangles``.  ``weld="device"``: they stay on the device and ``weldTrianglesDevice`` welds them
        there -- the same bytes, and only the V- and F-sized arrays of the result cross the bus.

        ``smooth=iterations``: the welded mesh goes through ``smoothMesh`` with its defaults -- before it is simplified: the
        fine mesh is denoised, then decimated -- and ``stats`` is added.  ``normals=True``: ``normals f32[V,3]``, ``vertexNormals`` of the final mesh,
        is added.  With ``weld="device"`` the positions stay on the device through both.

        ``simplify=cellSize``: the welded mesh goes through ``simplifyMesh`` on the grid of that cell size from the volume's
        origin, and its dict is returned (``faceMap``, ``vertexCluster`` and ``stats`` added); with ``weld="device"`` the welded mesh stays on the
        device until it is simplified.  With ``None``, ``None`` and ``False`` nothing more is launched."""
        if weld not in ("host", "device"):
            raise ValueError(f"extractMesh: weld must be 'host' or 'device', not {weld!r}")
        plain = smooth is None and not normals
        if weld == "host":
            mesh = weldTriangles(self.extractTriangles(minWeight))
            if plain:
                return mesh if simplify is None else simplifyMesh(self.device, mesh, simplify, self.origin)
            return finishMesh(self.device, mesh, self.origin, smooth, simplify, normals)
        tri = self.extractTriangleBuffers(minWeight)
        welded = {}
        try:
            if simplify is None and plain:
                return weldTrianglesDevice(self.device, tri)
            welded = weldTrianglesDevice(self.device, tri, asBuffers=True)
            if plain:
                return simplifyMesh(self.device, welded, simplify, self.origin)
            return finishMesh(self.device, welded, self.origin, smooth, simplify, normals, _read_welded)
        finally:
            destroyBuffers(tri)
            destroyBuffers(welded)

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_tsdf_volume_destroy(self.handle)
        self.handle = None


def weldTriangles(tri: dict) -> dict:
    """``TSDFVolume.extractTriangles``'s output as an indexed mesh (see ``TSDFVolume.extractMesh``).  Host side (numpy)."""
    keys = np.ascontiguousarray(tri["keys"], np.uint64).reshape(-1)
    uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    if uniq.size >= 2 ** 32:
        raise ValueError("weldTriangles: 2^32 vertices or more")
    vertices = np.ascontiguousarray(tri["positions"], np.float32).reshape(-1, 3)[first]
    colours = None if tri.get("colours") is None else np.ascontiguousarray(np.asarray(tri["colours"], np.uint8).reshape(-1, 4)[first, :3])
    return dict(vertices=np.ascontiguousarray(vertices), faces=inverse.reshape(-1, 3).astype(np.uint32), colours=colours, keys=uniq)


# ----------------------------------------------------------------------------- welding on the device (no reference counterpart)
def _read_welded(bufs: dict) -> dict:
    """The welded mesh ``weldTrianglesDevice(asBuffers=True)`` hands out, read back: ``dict(vertices, faces, colours u8[V,3] | None, keys)``."""
    V, F = bufs["numVertices"], bufs["numFaces"]
    colours = None if bufs["colours"] is None else np.ascontiguousarray(bufs["colours"].read(np.uint8, count=4 * V).reshape(V, 4)[:, :3])
    return dict(vertices=bufs["vertices"].read(np.float32, count=3 * V).reshape(V, 3), faces=bufs["faces"].read(np.uint32, count=3 * F).reshape(F, 3),
                colours=colours, keys=bufs["keys"].read(np.uint64, count=V))


def destroyBuffers(buffers: dict) -> None:
    """Destroys every ``HipBuffer`` among the values of ``buffers`` (the dicts ``extractTriangleBuffers`` and ``weldTrianglesDevice`` hand out)."""
    for b in buffers.values():
        if isinstance(b, HipBuffer):
            b.destroy()


class MeshWelder:
    """Welds a triangle soup on the device (``wdgs_mesh_welder``): ``count`` sorts the (key, slot) pairs with a stable radix sort, flags the first pair
    of every distinct key and returns their number (one wait); ``emit`` writes the indexed mesh.  ``weldTrianglesDevice`` is the one-call form;
    include/webdgs.h states the definition."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numSlots = self.numVertices = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_welder_create(device.handle, C.byref(h)))
        self.handle = h

    def count(self, keys: Optional[HipBuffer], numSlots: int) -> int:
        """The number of distinct keys among ``keys`` u64[numSlots], ``numSlots`` three per triangle and below 2^32 (sort, flags, scan; waits once)."""
        if not 0 <= int(numSlots) < 2 ** 64:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshWelder.count: bad slot count {numSlots}")
        if keys is not None and int(numSlots) < 2 ** 32 and keys.size < 8 * int(numSlots):
            raise ValueError("MeshWelder.count: buffer too small for the keys")
        n = C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_welder_count(self.handle, keys.ptr if keys is not None else None, int(numSlots), C.byref(n)))
        self.numSlots, self.numVertices = int(numSlots), int(n.value)
        return self.numVertices

    def emit(self, keys: Optional[HipBuffer], numSlots: int, positions: Optional[HipBuffer], colours: Optional[HipBuffer], facesOut: Optional[HipBuffer],
             verticesOut: Optional[HipBuffer] = None, coloursOut: Optional[HipBuffer] = None, keysOut: Optional[HipBuffer] = None,
             capacity: Optional[int] = None) -> None:
        """Writes ``facesOut`` u32[numSlots], ``verticesOut`` f32[V][3] gathered from ``positions`` f32[numSlots][3], ``coloursOut`` rgba8[V] gathered from
        ``colours`` rgba8[numSlots] and ``keysOut`` u64[V] for the count before it (``StateError`` otherwise; ``CapacityError``, with nothing written, when
        there is room for fewer than V vertices).  Stream-ordered: it waits for nothing and records."""
        outs = ((verticesOut, 12), (coloursOut, 4), (keysOut, 8))
        cap = min([b.size // s for b, s in outs if b is not None] or [2 ** 32 - 1]) if capacity is None else int(capacity)
        for b, s in outs:
            if b is not None and cap * s > b.size:
                raise ValueError("MeshWelder.emit: the capacity exceeds the buffers")
        n = int(numSlots)
        if n < 2 ** 32 and ((facesOut is not None and facesOut.size < 4 * n) or (positions is not None and positions.size < 12 * n)
                            or (colours is not None and colours.size < 4 * n)):
            raise ValueError("MeshWelder.emit: buffers too small for the slots")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_welder_emit(self.handle, ptr(keys), n, ptr(positions), ptr(colours), ptr(keysOut), ptr(verticesOut), ptr(coloursOut),
                                                    ptr(facesOut), cap))

    def stats(self) -> dict:
        """The last count: ``dict(passesRun, passesSkipped, vertices, slots)`` -- of the eight radix passes, those whose digit differs somewhere ran.  The
        kernels' event times are ``HipDevice.kernelTimes``' (``weld_*`` and the scan's)."""
        v = [C.c_uint32(0) for _ in range(4)]
        check(self.device.lib.wdgs_mesh_welder_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(passesRun=int(v[0].value), passesSkipped=int(v[1].value), vertices=int(v[2].value), slots=int(v[3].value))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_welder_destroy(self.handle)
        self.handle = None


def weldTrianglesDevice(device: HipDevice, tri: dict, asBuffers: bool = False) -> dict:
    """``weldTriangles`` on the device, byte for byte: ``tri`` is ``extractTriangles``'s numpy dict (uploaded) or ``extractTriangleBuffers``'s dict of
    ``HipBuffer`` plus ``numTriangles`` (left as it is); returns ``dict(vertices f32[V,3], faces u32[F,3], colours u8[V,3] | None, keys u64[V])``.  A vertex
    takes the position and colour of the lowest slot that carries its key.  ``asBuffers``: ``vertices`` f32[V][3], ``faces`` u32[F][3], ``keys`` u64[V] and
    ``colours`` rgba8[V] (or ``None``) stay on the device as ``HipBuffer`` of exactly those sizes -- what ``meshComponents``, ``removeSmallComponents``
    and ``sampleMesh`` take -- and ``numVertices`` and ``numFaces`` are added; the caller destroys them (``destroyBuffers``)."""
    own = not isinstance(tri["keys"], HipBuffer)
    if own:
        k = np.ascontiguousarray(tri["keys"], np.uint64).reshape(-1)
        if k.size % 3:
            raise ValueError("weldTrianglesDevice: the keys are not three per triangle")
        F = k.size // 3
        p = np.ascontiguousarray(tri["positions"], np.float32).reshape(-1)
        c = None if tri.get("colours") is None else np.ascontiguousarray(tri["colours"], np.uint8).reshape(-1)
        if p.size != 9 * F or (c is not None and c.size != 12 * F):
            raise ValueError("weldTrianglesDevice: positions or colours disagree with the keys")
        src = dict(keys=device.bufferFrom(k), positions=device.bufferFrom(p), colours=None if c is None else device.bufferFrom(c))
    else:
        F = int(tri["numTriangles"])
        src = dict(keys=tri["keys"], positions=tri["positions"], colours=tri.get("colours"))
    S = 3 * F
    welder = MeshWelder(device)
    out = {}
    try:
        V = welder.count(src["keys"], S)
        out = dict(vertices=device.createBuffer(12 * V, "welded vertices"), faces=device.createBuffer(4 * S, "welded faces"),
                   colours=None if src["colours"] is None else device.createBuffer(4 * V, "welded colours"), keys=device.createBuffer(8 * V, "welded keys"))
        welder.emit(src["keys"], S, src["positions"], src["colours"], out["faces"], out["vertices"], out["colours"], out["keys"], V)
        if asBuffers:
            device.synchronize()   # (an uploaded soup is released below)
            result, out = dict(out, numVertices=V, numFaces=F), {}
            return result
        return _read_welded(dict(out, numVertices=V, numFaces=F))
    finally:
        welder.destroy()
        destroyBuffers(out)
        if own:
            destroyBuffers(src)


# ----------------------------------------------------------------------------- simplification by vertex clustering (no reference counterpart)
class MeshSimplifier:
    """Simplifies an indexed mesh on the device by vertex clustering (``wdgs_mesh_simplifier``): ``count`` keys every vertex by its cell of the grid
    ``(origin, cellSize)``, numbers the clusters, reduces each to one representative, drops the faces that are invalid, outside, collapsed or
    duplicates and returns ``(V', F')`` (one wait); ``emit`` writes the simplified mesh.  ``simplifyMesh`` is the one-call form; include/webdgs.h
    states the definition."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numVertices = self.numFaces = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_simplifier_create(device.handle, C.byref(h)))
        self.handle = h

    def count(self, vertices: Optional[HipBuffer], numVertices: int, faces: Optional[HipBuffer], numFaces: int, colours: Optional[HipBuffer], origin,
              cellSize: float) -> tuple:
        """``(V', F')`` for ``vertices`` f32[numVertices][3], ``faces`` u32[numFaces][3] and (optional) ``colours`` rgba8[numVertices] (keys, sorts, sums,
        classes, flags, scans; waits once)."""
        nv, nf = int(numVertices), int(numFaces)
        if not (0 <= nv < 2 ** 32 and 0 <= nf < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshSimplifier.count: bad counts {numVertices}, {numFaces}")
        if nv < 2 ** 31 and nf < 2 ** 31 and ((vertices is not None and vertices.size < 12 * nv) or (faces is not None and faces.size < 12 * nf)
                                              or (colours is not None and colours.size < 4 * nv)):
            raise ValueError("MeshSimplifier.count: buffers too small for the mesh")
        o = (C.c_float * 3)(*[float(x) for x in np.asarray(origin, np.float32).reshape(3)])
        ptr = lambda b: b.ptr if b is not None else None
        v, f = C.c_uint32(0), C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_simplifier_count(self.handle, ptr(vertices), nv, ptr(faces), nf, ptr(colours), o, float(cellSize), C.byref(v), C.byref(f)))
        self.numVertices, self.numFaces = int(v.value), int(f.value)
        return self.numVertices, self.numFaces

    def emit(self, vertices: Optional[HipBuffer], numVertices: int, faces: Optional[HipBuffer], numFaces: int, colours: Optional[HipBuffer],
             verticesOut: Optional[HipBuffer], facesOut: Optional[HipBuffer], coloursOut: Optional[HipBuffer] = None, keysOut: Optional[HipBuffer] = None,
             faceMap: Optional[HipBuffer] = None, vertexCluster: Optional[HipBuffer] = None, capacityVertices: Optional[int] = None,
             capacityFaces: Optional[int] = None) -> None:
        """Writes ``verticesOut`` f32[V'][3], ``facesOut`` u32[F'][3], ``coloursOut`` rgba8[V'], ``keysOut`` u64[V'], ``faceMap`` u32[F'] and
        ``vertexCluster`` u32[numVertices] for the count before it (``StateError`` otherwise; ``CapacityError``, with nothing written, when there is
        room for fewer than V' vertices or F' faces).  Stream-ordered: it waits for nothing and records."""
        vouts, fouts = ((verticesOut, 12), (coloursOut, 4), (keysOut, 8)), ((facesOut, 12), (faceMap, 4))
        cv = min([b.size // s for b, s in vouts if b is not None] or [2 ** 32 - 1]) if capacityVertices is None else int(capacityVertices)
        cf = min([b.size // s for b, s in fouts if b is not None] or [2 ** 32 - 1]) if capacityFaces is None else int(capacityFaces)
        for outs, cap in ((vouts, cv), (fouts, cf)):
            for b, s in outs:
                if b is not None and cap * s > b.size:
                    raise ValueError("MeshSimplifier.emit: the capacity exceeds the buffers")
        if vertexCluster is not None and vertexCluster.size < 4 * int(numVertices):
            raise ValueError("MeshSimplifier.emit: vertexCluster is too small for the vertices")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_simplifier_emit(self.handle, ptr(vertices), int(numVertices), ptr(faces), int(numFaces), ptr(colours), ptr(verticesOut),
                                                        ptr(coloursOut), ptr(keysOut), ptr(facesOut), ptr(faceMap), ptr(vertexCluster), cv, cf))

    def stats(self) -> dict:
        """The last count: ``dict(clusters, invalid, outside, collapsed, duplicate, vertices, faces)`` -- the occupied cells, the dropped faces by class,
        V' and F'.  The kernels' event times are ``HipDevice.kernelTimes``' (``simplify_*``, ``weld_*`` and the scan's)."""
        v = [C.c_uint32(0) for _ in range(7)]
        check(self.device.lib.wdgs_mesh_simplifier_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("clusters", "invalid", "outside", "collapsed", "duplicate", "vertices", "faces"), (int(x.value) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_simplifier_destroy(self.handle)
        self.handle = None


def _read_simplified(bufs: dict, V: int) -> dict:
    """The mesh ``simplifyMesh(asBuffers=True)`` hands out for an input of ``V`` vertices, read back as ``simplifyMesh`` returns it."""
    nv, nf = bufs["numVertices"], bufs["numFaces"]
    colours = None if bufs["colours"] is None else np.ascontiguousarray(bufs["colours"].read(np.uint8, count=4 * nv).reshape(nv, 4)[:, :3])
    return dict(vertices=bufs["vertices"].read(np.float32, count=3 * nv).reshape(nv, 3), faces=bufs["faces"].read(np.uint32, count=3 * nf).reshape(nf, 3),
                colours=colours, keys=bufs["keys"].read(np.uint64, count=nv), faceMap=bufs["faceMap"].read(np.uint32, count=nf),
                vertexCluster=bufs["vertexCluster"].read(np.uint32, count=V), stats=bufs["stats"])


def simplifyMesh(device: HipDevice, mesh: dict, cellSize: float, origin=None, asBuffers: bool = False) -> dict:
    """``mesh`` simplified by vertex clustering on a grid of ``cellSize`` from ``origin``: the vertices of one cell become one vertex at the integer mean
    of their sub-cell offsets (colours alike), faces that collapse or repeat a lower face's cluster triple are dropped, unreferenced clusters are left
    out.  ``mesh`` is the dict ``extractMesh`` / ``loaders.loadMeshPLY`` return (uploaded; colours u8[V,3] get an alpha of 255, u8[V,4] go as they are),
    or a dict of ``HipBuffer``s -- ``vertices`` f32[V][3], ``faces`` u32[F][3], ``colours`` rgba8[V] or ``None``, with ``numVertices`` / ``numFaces``
    or whole buffers -- as ``weldTrianglesDevice(asBuffers=True)`` hands out (left as it is).  ``origin=None``: the per-axis minimum of the finite
    vertices (numpy input only; a device mesh needs an origin: ``ValueError``).  Returns ``dict(vertices f32[V',3], faces u32[F',3], colours u8[V',3] |
    None, keys u64[V'], faceMap u32[F'], vertexCluster u32[V], stats)``; a function of its arguments alone, bit for bit (include/webdgs.h states it).
    ``asBuffers``: ``vertices``, ``faces``, ``colours`` (rgba8[V']), ``keys``, ``faceMap`` and ``vertexCluster`` stay on the device as ``HipBuffer`` of
    exactly those sizes -- what ``meshComponents``, ``sampleMesh`` and another ``simplifyMesh`` take -- and ``numVertices`` and ``numFaces`` are added;
    the caller destroys them (``destroyBuffers``)."""
    own = not isinstance(mesh["vertices"], HipBuffer)
    if own:
        v = np.ascontiguousarray(mesh["vertices"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.uint32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"simplifyMesh: expected vertices [V, 3] and faces [F, 3], got {v.shape} and {f.shape}")
        c = None
        if mesh.get("colours") is not None:
            c = np.ascontiguousarray(mesh["colours"], np.uint8)
            if c.ndim != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4):
                raise ValueError(f"simplifyMesh: colours of shape {c.shape} for {v.shape[0]} vertices")
            if c.shape[1] == 3:
                c = np.ascontiguousarray(np.concatenate([c, np.full((c.shape[0], 1), 255, np.uint8)], axis=1))
        if origin is None:
            finite = v[np.all(np.isfinite(v), axis=1)]
            origin = finite.min(axis=0) if finite.shape[0] else np.zeros(3, np.float32)
        V, F = v.shape[0], f.shape[0]
        src = dict(vertices=device.bufferFrom(v, "simplifyMesh: vertices"), faces=device.bufferFrom(f, "simplifyMesh: faces"),
                   colours=None if c is None else device.bufferFrom(c, "simplifyMesh: colours"))
    else:
        if origin is None:
            raise ValueError("simplifyMesh: a mesh on the device needs an explicit origin")
        if not isinstance(mesh["faces"], HipBuffer) or not (mesh.get("colours") is None or isinstance(mesh["colours"], HipBuffer)):
            raise ValueError("simplifyMesh: vertices on the device need faces and colours on the device")
        V = int(mesh["numVertices"]) if "numVertices" in mesh else mesh["vertices"].size // 12
        F = int(mesh["numFaces"]) if "numFaces" in mesh else mesh["faces"].size // 12
        src = dict(vertices=mesh["vertices"], faces=mesh["faces"], colours=mesh.get("colours"))
    simplifier = MeshSimplifier(device)
    out = {}
    try:
        nv, nf = simplifier.count(src["vertices"], V, src["faces"], F, src["colours"], origin, cellSize)
        out = dict(vertices=device.createBuffer(12 * nv, "simplified vertices"), faces=device.createBuffer(12 * nf, "simplified faces"),
                   colours=None if src["colours"] is None else device.createBuffer(4 * nv, "simplified colours"), keys=device.createBuffer(8 * nv, "simplified keys"),
                   faceMap=device.createBuffer(4 * nf, "simplified face map"), vertexCluster=device.createBuffer(4 * V, "simplified vertex clusters"))
        simplifier.emit(src["vertices"], V, src["faces"], F, src["colours"], out["vertices"], out["faces"], out["colours"], out["keys"], out["faceMap"],
                        out["vertexCluster"], nv, nf)
        stats = simplifier.stats()
        if asBuffers:
            device.synchronize()   # (an uploaded mesh is released below)
            result, out = dict(out, numVertices=nv, numFaces=nf, stats=stats), {}
            return result
        return _read_simplified(dict(out, numVertices=nv, numFaces=nf, stats=stats), V)
    finally:
        simplifier.destroy()
        destroyBuffers(out)
        if own:
            destroyBuffers(src)


# ----------------------------------------------------------------------------- adjacency, smoothing and vertex normals (no reference counterpart)
SMOOTH_PIN_BOUNDARY = 1   # WDGS_SMOOTH_PIN_BOUNDARY
ADJACENCY_STATS = ("directedEdges", "edges", "boundaryEdges", "nonManifoldEdges", "invalidFaces", "boundaryVertices", "isolatedVertices", "maxDegree")


class MeshAdjacency:
    """The per-vertex neighbour lists of an indexed mesh on the device (``wdgs_mesh_adjacency``) and what stands on them: ``count`` sorts the faces'
    directed half-edge keys (the welder's stable u64 sort over ``6 F`` slots), delimits the rows, flags the boundary and returns ``E`` (one wait);
    ``emit`` writes ``rowStart``, ``neighbours`` and ``boundary``; ``smooth`` runs Taubin's lambda | mu steps and ``normals`` the area-weighted vertex
    normals over that count, both stream-ordered.  ``meshAdjacency``, ``smoothMesh`` and ``vertexNormals`` are the one-call forms; include/webdgs.h
    states the definition."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numEdges = self.numVertices = self.numFaces = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_adjacency_create(device.handle, C.byref(h)))
        self.handle = h

    def count(self, faces: Optional[HipBuffer], numFaces: int, numVertices: int) -> int:
        """``E``, the number of directed edges of ``faces`` u32[numFaces][3] over ``numVertices`` vertices (keys, sort, rows, flags, statistics; waits
        once).  The faces must stay as they are while ``normals`` may still be called."""
        nf, nv = int(numFaces), int(numVertices)
        if not (0 <= nv < 2 ** 32 and 0 <= nf < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshAdjacency.count: bad counts {numVertices}, {numFaces}")
        if 6 * nf < 2 ** 32 and faces is not None and faces.size < 12 * nf:
            raise ValueError("MeshAdjacency.count: buffer too small for the faces")
        e = C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_adjacency_count(self.handle, faces.ptr if faces is not None else None, nf, nv, C.byref(e)))
        self.numEdges, self.numVertices, self.numFaces = int(e.value), nv, nf
        return self.numEdges

    def emit(self, rowStart: Optional[HipBuffer] = None, neighbours: Optional[HipBuffer] = None, boundary: Optional[HipBuffer] = None,
             capacityEdges: Optional[int] = None) -> None:
        """Writes ``rowStart`` u32[V + 1], ``neighbours`` u32[E] and ``boundary`` u32[V] of the count before it, each optional (``StateError`` without a
        count; ``CapacityError``, with nothing written, when there is room for fewer than E edges).  Stream-ordered: it waits for nothing and records."""
        cap = (neighbours.size // 4 if neighbours is not None else 2 ** 32 - 1) if capacityEdges is None else int(capacityEdges)
        if neighbours is not None and 4 * cap > neighbours.size:
            raise ValueError("MeshAdjacency.emit: the capacity exceeds the buffer")
        if (rowStart is not None and rowStart.size < 4 * (self.numVertices + 1)) or (boundary is not None and boundary.size < 4 * self.numVertices):
            raise ValueError("MeshAdjacency.emit: buffers too small for the vertices")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_adjacency_emit(self.handle, ptr(rowStart), ptr(neighbours), ptr(boundary), cap))

    def smooth(self, verticesIn: Optional[HipBuffer], verticesOut: Optional[HipBuffer], numVertices: int, iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
               pinBoundary: bool = True) -> None:
        """``verticesOut`` f32[V][3] = ``verticesIn`` after ``iterations`` rounds of ``step(lam)`` then ``step(mu)`` over the counted adjacency (a weight of
        exactly 0 skips its step; ``verticesOut`` may be ``verticesIn``).  ``StateError`` unless ``numVertices`` is the count's.  Stream-ordered: it
        waits for nothing, allocates nothing and records."""
        nv, it = int(numVertices), int(iterations)
        if not (0 <= nv < 2 ** 32 and 0 <= it < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshAdjacency.smooth: bad counts {numVertices}, {iterations}")
        for b in (verticesIn, verticesOut):
            if b is not None and nv == self.numVertices and b.size < 12 * nv:
                raise ValueError("MeshAdjacency.smooth: buffer too small for the vertices")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_adjacency_smooth(self.handle, ptr(verticesIn), ptr(verticesOut), nv, it, float(lam), float(mu),
                                                         SMOOTH_PIN_BOUNDARY if pinBoundary else 0))

    def normals(self, vertices: Optional[HipBuffer], faces: Optional[HipBuffer], numVertices: int, numFaces: int, normalsOut: Optional[HipBuffer]) -> None:
        """``normalsOut`` f32[V][3]: the area-weighted normals of ``vertices`` f32[V][3] over the counted faces -- ``faces`` must be the buffer that was
        counted, unchanged (``StateError`` otherwise).  Stream-ordered: it waits for nothing and records."""
        nv = int(numVertices)
        for b in (vertices, normalsOut):
            if b is not None and nv == self.numVertices and b.size < 12 * nv:
                raise ValueError("MeshAdjacency.normals: buffer too small for the vertices")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_adjacency_normals(self.handle, ptr(vertices), ptr(faces), nv, int(numFaces), ptr(normalsOut)))

    def stats(self) -> dict:
        """The last count: ``dict(directedEdges, edges, boundaryEdges, nonManifoldEdges, invalidFaces, boundaryVertices, isolatedVertices, maxDegree)``.
        The kernels' event times are ``HipDevice.kernelTimes``' (``adjacency_*``, ``weld_*`` and the scan's)."""
        v = [C.c_uint32(0) for _ in ADJACENCY_STATS]
        check(self.device.lib.wdgs_mesh_adjacency_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(ADJACENCY_STATS, (int(x.value) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_adjacency_destroy(self.handle)
        self.handle = None


def _mesh_on_device(device: HipDevice, mesh: dict, what: str) -> tuple:
    """``(vertices, faces, V, F, own)``: the mesh's positions and faces as ``HipBuffer`` -- uploaded from numpy (``own``: the caller destroys them) or
    taken as they are from a dict of buffers with ``numVertices`` / ``numFaces`` or whole buffers."""
    if not isinstance(mesh["vertices"], HipBuffer):
        v = np.ascontiguousarray(mesh["vertices"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.uint32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"{what}: expected vertices [V, 3] and faces [F, 3], got {v.shape} and {f.shape}")
        return device.bufferFrom(v, f"{what}: vertices"), device.bufferFrom(f, f"{what}: faces"), v.shape[0], f.shape[0], True
    if not isinstance(mesh["faces"], HipBuffer):
        raise ValueError(f"{what}: vertices on the device need faces on the device")
    V = int(mesh["numVertices"]) if "numVertices" in mesh else mesh["vertices"].size // 12
    F = int(mesh["numFaces"]) if "numFaces" in mesh else mesh["faces"].size // 12
    return mesh["vertices"], mesh["faces"], V, F, False


def meshAdjacency(device: HipDevice, mesh: dict) -> dict:
    """The neighbour lists of ``mesh`` (numpy, or a dict of ``HipBuffer`` as ``weldTrianglesDevice(asBuffers=True)`` hands out; only ``faces`` and the
    vertex count matter): ``dict(rowStart u32[V+1], neighbours u32[E], boundary u32[V], stats)`` -- vertex ``v`` neighbours
    ``neighbours[rowStart[v]:rowStart[v+1]]``, ascending; ``boundary`` is 1 on both ends of every edge that one face alone holds; ``stats`` is
    ``MeshAdjacency.stats``'s dict.  A function of the faces alone, bit for bit (include/webdgs.h states it)."""
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, "meshAdjacency")
    adjacency = MeshAdjacency(device)
    out = {}
    try:
        E = adjacency.count(faces, F, V)
        out = dict(rowStart=device.createBuffer(4 * (V + 1), "adjacency row starts"), neighbours=device.createBuffer(4 * E, "adjacency neighbours"),
                   boundary=device.createBuffer(4 * V, "adjacency boundary flags"))
        adjacency.emit(out["rowStart"], out["neighbours"], out["boundary"], E)
        return dict(rowStart=out["rowStart"].read(np.uint32, count=V + 1), neighbours=out["neighbours"].read(np.uint32, count=E),
                    boundary=out["boundary"].read(np.uint32, count=V), stats=adjacency.stats())
    finally:
        adjacency.destroy()
        destroyBuffers(out)
        if own:
            vertices.destroy()
            faces.destroy()


def _smooth_and_normals(device: HipDevice, vertices: HipBuffer, faces: HipBuffer, V: int, F: int, smooth, normals: bool, lam: float = 0.5, mu: float = -0.53,
                        pinBoundary: bool = True) -> tuple:
    """``(smoothed | None, normals | None, stats)`` of a mesh on the device through one ``MeshAdjacency``: a new buffer of the positions after ``smooth``
    iterations (``None``: not wanted) and a new buffer of the normals of the smoothed -- else the given -- positions.  The caller destroys both."""
    adjacency = MeshAdjacency(device)
    out = {}
    try:
        adjacency.count(faces, F, V)
        if smooth is not None:
            out["smoothed"] = device.createBuffer(12 * V, "smoothed vertices")
            adjacency.smooth(vertices, out["smoothed"], V, smooth, lam, mu, pinBoundary)
        if normals:
            out["normals"] = device.createBuffer(12 * V, "vertex normals")
            adjacency.normals(out.get("smoothed", vertices), faces, V, F, out["normals"])
        stats = adjacency.stats()
        device.synchronize()   # (the object's arrays are released below)
        result, out = (out.get("smoothed"), out.get("normals"), stats), {}
        return result
    finally:
        adjacency.destroy()
        destroyBuffers(out)


def smoothMesh(device: HipDevice, mesh: dict, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, pinBoundary: bool = True, asBuffers: bool = False) -> dict:
    """``mesh`` after ``iterations`` rounds of Taubin's lambda | mu smoothing (``mu = 0``: plain Laplacian smoothing): every vertex moves towards, then
    away from, the f32 mean of its neighbours, summed in ascending neighbour order; with ``pinBoundary`` the ends of boundary edges stay where they are.
    ``mesh`` is the dict ``extractMesh`` / ``loaders.loadMeshPLY`` return, or a dict of ``HipBuffer``s as ``weldTrianglesDevice(asBuffers=True)`` and
    ``simplifyMesh(asBuffers=True)`` hand out (left as it is).  Returns the mesh's dict with new ``vertices``, every other entry passed through, and
    ``stats`` (``MeshAdjacency.stats``) added; a function of its arguments alone, bit for bit (include/webdgs.h states it).  ``asBuffers``: ``vertices``
    is a new ``HipBuffer`` f32[V][3] the caller destroys; a numpy mesh's ``faces`` are then handed out as a buffer too, with ``numVertices`` and
    ``numFaces`` added."""
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, "smoothMesh")
    smoothed = None
    try:
        smoothed, _, stats = _smooth_and_normals(device, vertices, faces, V, F, iterations, False, lam, mu, pinBoundary)
        if asBuffers:
            result = dict(mesh, vertices=smoothed, stats=stats, numVertices=V, numFaces=F)
            if own:
                result["faces"], faces = faces, None
            smoothed = None
            return result
        return dict(mesh, vertices=smoothed.read(np.float32, count=3 * V).reshape(V, 3), stats=stats)
    finally:
        if smoothed is not None:
            smoothed.destroy()
        if own:
            vertices.destroy()
            if faces is not None:
                faces.destroy()


def vertexNormals(device: HipDevice, mesh: dict) -> np.ndarray:
    """The area-weighted unit normals ``f32[V,3]`` of ``mesh`` (numpy or a dict of ``HipBuffer``s): per vertex the sum of its faces' cross products in the
    order the half-edge sort fixes, normalised; ``(0, 0, 0)`` for a vertex without a face of non-zero finite area.  A function of the mesh alone, bit for
    bit (include/webdgs.h states it)."""
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, "vertexNormals")
    normals = None
    try:
        _, normals, _ = _smooth_and_normals(device, vertices, faces, V, F, None, True)
        return normals.read(np.float32, count=3 * V).reshape(V, 3)
    finally:
        if normals is not None:
            normals.destroy()
        if own:
            vertices.destroy()
            faces.destroy()


def finishMesh(device: HipDevice, mesh: dict, origin, smooth: Optional[int], simplify: Optional[float], normals: bool, read=None) -> dict:
    """What ``extractMesh`` does to a welded (and compacted) mesh, in its order: ``smoothMesh(mesh, smooth)`` when ``smooth`` is not ``None``, then
    ``simplifyMesh(mesh, simplify, origin)`` when ``simplify`` is not ``None``, then ``normals = vertexNormals(mesh)`` when asked for; returned as numpy.
    A numpy ``mesh`` goes through the three functions as they are.  A mesh of ``HipBuffer``s with ``numVertices`` and ``numFaces`` stays on the device
    throughout: its ``vertices`` buffer is replaced by the smoothed one (the caller still destroys the dict), and ``read(mesh)`` turns it into the numpy
    dict to return when it is not simplified."""
    if not isinstance(mesh["vertices"], HipBuffer):
        if smooth is not None:
            mesh = smoothMesh(device, mesh, smooth)
        if simplify is not None:
            mesh = simplifyMesh(device, mesh, simplify, origin)
        return dict(mesh, normals=vertexNormals(device, mesh)) if normals else mesh
    V, F = int(mesh["numVertices"]), int(mesh["numFaces"])

    def normals_of(buf) -> np.ndarray:
        try:
            return buf.read(np.float32, count=buf.size // 4).reshape(-1, 3)
        finally:
            buf.destroy()

    stats = vn = None
    if smooth is not None or (normals and simplify is None):
        smoothed, nbuf, stats = _smooth_and_normals(device, mesh["vertices"], mesh["faces"], V, F, smooth, normals and simplify is None)
        if smoothed is not None:
            mesh["vertices"].destroy()
            mesh["vertices"] = smoothed
        if nbuf is not None:
            vn = normals_of(nbuf)
    if simplify is None:
        out = read(mesh)
        if smooth is not None:
            out["stats"] = stats
        if normals:
            out["normals"] = vn
        return out
    if not normals:
        return simplifyMesh(device, mesh, simplify, origin)
    simplified = simplifyMesh(device, mesh, simplify, origin, asBuffers=True)
    try:
        out = _read_simplified(simplified, V)
        _, nbuf, _ = _smooth_and_normals(device, simplified["vertices"], simplified["faces"], simplified["numVertices"], simplified["numFaces"], None, True)
        out["normals"] = normals_of(nbuf)
        return out
    finally:
        destroyBuffers(simplified)


# ----------------------------------------------------------------------------- mesh rasterization and depth agreement (no reference counterpart)
CULL_MODES = {"none": 0, "back": 1, "front": 2}   # WDGS_CULL_NONE, WDGS_CULL_BACK, WDGS_CULL_FRONT
MESH_RASTER_LARGE_FACE_PIXELS = _lib.MESH_RASTER_LARGE_FACE_PIXELS
# the depth below which the forward pass drops a Gaussian: csrc/project.hip, project_one, `ndc.z < 0.0f`, which synth.projection_matrix's znear = 0.01 puts there
MESH_RASTER_NEAR = 0.01
RASTER_STATS = ("invalidFaces", "clippedFaces", "degenerateFaces", "culledFaces", "emptyFaces", "rasterizedFaces", "coveredPixels", "viewportMismatch")
RASTER_OUTPUTS = {"depth": (4, np.float32), "face": (4, np.uint32), "colour": (4, np.uint8), "normal": (16, np.float32)}   # bytes per pixel, read-back type
NO_FACE = 0xFFFFFFFF


class MeshRasterizer:
    """A z-buffered triangle rasterizer under the library's camera block (``wdgs_mesh_rasterizer``): ``encode`` draws an indexed mesh on the device into
    the depth, face, colour and normal images asked for, ``stats`` reads the face classes and the covered pixels of the last encode.  Every byte is a
    function of the input alone (include/webdgs.h states the definition; coverage in integers, one 64-bit atomic min per fragment).  There is no
    clipping: a face with a vertex nearer than ``near`` is dropped whole.  ``rasterizeMesh`` is the one-call form."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_rasterizer_create(device.handle, C.byref(h)))
        self.handle = h

    def encode(self, vertices: Optional[HipBuffer], numVertices: int, faces: Optional[HipBuffer], numFaces: int, colours: Optional[HipBuffer], camera: HipBuffer,
               width: int, height: int, near: float = MESH_RASTER_NEAR, cull: str = "none", depth: Optional[HipBuffer] = None, face: Optional[HipBuffer] = None,
               colour: Optional[HipBuffer] = None, normal: Optional[HipBuffer] = None) -> None:
        """Draws ``vertices`` f32[numVertices][3], ``faces`` u32[numFaces][3] (and ``colours`` rgba8[numVertices] for a colour image) under ``camera``
        (the 68-float block on the device) into ``depth`` f32, ``face`` u32, ``colour`` rgba8 and ``normal`` rgba32f images of ``width`` x ``height``, each
        optional.  Stream-ordered: it waits for nothing and records -- except a call that has to grow the object's arrays (``StateError`` while
        recording; encode once eagerly first)."""
        nv, nf, w, h = int(numVertices), int(numFaces), int(width), int(height)
        if cull not in CULL_MODES:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshRasterizer.encode: unknown cull mode {cull!r} (none, back, front)")
        if not (0 <= nv < 2 ** 32 and 0 <= nf < 2 ** 32 and 0 <= w < 2 ** 32 and 0 <= h < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshRasterizer.encode: bad counts {numVertices}, {numFaces}, {width}x{height}")
        if nv < 2 ** 31 and 3 * nf < 2 ** 32 and ((vertices is not None and vertices.size < 12 * nv) or (faces is not None and faces.size < 12 * nf)
                                                 or (colours is not None and colours.size < 4 * nv)):
            raise ValueError("MeshRasterizer.encode: buffers too small for the mesh")
        if camera.size < 272:
            raise ValueError("MeshRasterizer.encode: the camera block has 68 floats")
        if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE:
            for name, buf in (("depth", depth), ("face", face), ("colour", colour), ("normal", normal)):
                if buf is not None and buf.size < RASTER_OUTPUTS[name][0] * w * h:
                    raise ValueError(f"MeshRasterizer.encode: the {name} image is too small for {w}x{h}")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_rasterizer_encode(self.handle, ptr(vertices), nv, ptr(faces), nf, ptr(colours), camera.ptr, w, h, float(near), CULL_MODES[cull],
                                                          ptr(depth), ptr(face), ptr(colour), ptr(normal)))

    def stats(self) -> dict:
        """The last encode: ``dict(invalidFaces, clippedFaces, degenerateFaces, culledFaces, emptyFaces, rasterizedFaces, coveredPixels, viewportMismatch)``
        -- every face is in exactly one class.  Waits (``StateError`` before an encode and while recording)."""
        v = [C.c_uint32(0) for _ in RASTER_STATS]
        check(self.device.lib.wdgs_mesh_rasterizer_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(RASTER_STATS, (int(x.value) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_rasterizer_destroy(self.handle)
        self.handle = None


def _mesh_colours_on_device(device: HipDevice, mesh: dict, V: int, own: bool, what: str) -> tuple:
    """``(colours | None, owned)``: the mesh's vertex colours as an rgba8[V] ``HipBuffer`` -- a numpy mesh's u8[V,3] get an alpha of 255, as ``simplifyMesh``
    uploads them."""
    c = mesh.get("colours")
    if c is None:
        return None, False
    if isinstance(c, HipBuffer):
        if own:
            raise ValueError(f"{what}: colours on the device need vertices on the device")
        return c, False
    if not own:
        raise ValueError(f"{what}: vertices on the device need colours on the device")
    c = np.ascontiguousarray(c, np.uint8)
    if c.ndim != 2 or c.shape[0] != V or c.shape[1] not in (3, 4):
        raise ValueError(f"{what}: colours of shape {c.shape} for {V} vertices")
    if c.shape[1] == 3:
        c = np.ascontiguousarray(np.concatenate([c, np.full((V, 1), 255, np.uint8)], axis=1))
    return device.bufferFrom(c, f"{what}: colours"), True


def _camera_on_device(device: HipDevice, camera, what: str) -> tuple:
    if isinstance(camera, HipBuffer):
        return camera, False
    c = np.ascontiguousarray(camera, np.float32).reshape(-1)
    if c.size != 68:
        raise ValueError(f"{what}: the camera block has 68 floats, got {c.size}")
    return device.bufferFrom(c, f"{what}: camera"), True


def rasterizeMesh(device: HipDevice, mesh: dict, camera, width: int, height: int, near: float = MESH_RASTER_NEAR, cull: str = "none", outputs=("depth", "face"),
                  asBuffers: bool = False) -> dict:
    """The images of ``mesh`` under ``camera`` (the 68-float block, numpy or ``HipBuffer``): ``dict(depth f32[H,W], face u32[H,W], colour u8[H,W,4], normal
    f32[H,W,4], stats)`` with the ``outputs`` asked for.  ``mesh`` is the dict ``extractMesh`` / ``loaders.loadMeshPLY`` return, or a dict of ``HipBuffer``s
    as ``weldTrianglesDevice(asBuffers=True)`` and ``simplifyMesh(asBuffers=True)`` hand out (left as it is); ``colour`` needs its ``colours``.  A pixel no
    face covers has depth 0, face ``NO_FACE``, colour and normal all zero.  ``near`` defaults to the depth below which the forward pass drops a Gaussian, so
    mesh and model are clipped alike -- by dropping, not by cutting: a face with a vertex nearer than ``near`` is not drawn.  ``cull``: ``"none"``,
    ``"back"`` or ``"front"``.  A function of its arguments alone, bit for bit (include/webdgs.h states it).  ``asBuffers``: the images stay on the device
    as ``HipBuffer`` the caller destroys."""
    outputs = tuple(outputs)
    for name in outputs:
        if name not in RASTER_OUTPUTS:
            raise ValueError(f"rasterizeMesh: unknown output {name!r} (depth, face, colour, normal)")
    w, h = int(width), int(height)
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, "rasterizeMesh")
    colours = cam = None
    own_colours = own_cam = False
    rasterizer = None
    out = {}
    try:
        if "colour" in outputs:
            colours, own_colours = _mesh_colours_on_device(device, mesh, V, own, "rasterizeMesh")
            if colours is None:
                raise _lib.WdgsError(_lib.WDGS_E_INVALID, "rasterizeMesh: a colour image needs a mesh with colours")
        cam, own_cam = _camera_on_device(device, camera, "rasterizeMesh")
        rasterizer = MeshRasterizer(device)
        npix = w * h if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE else 0
        out = {name: device.createBuffer(RASTER_OUTPUTS[name][0] * npix, f"mesh {name} image") for name in outputs}
        rasterizer.encode(vertices, V, faces, F, colours, cam, w, h, near, cull, **out)
        stats = rasterizer.stats()
        if asBuffers:
            result, out = dict(out, stats=stats), {}
            return result
        shapes = {"depth": (h, w), "face": (h, w), "colour": (h, w, 4), "normal": (h, w, 4)}
        return dict({name: out[name].read(RASTER_OUTPUTS[name][1], count=int(np.prod(shapes[name]))).reshape(shapes[name]) for name in outputs}, stats=stats)
    finally:
        if rasterizer is not None:
            rasterizer.destroy()
        destroyBuffers(out)
        if own:
            vertices.destroy()
            faces.destroy()
        if own_colours:
            colours.destroy()
        if own_cam:
            cam.destroy()


def faceIndexColours(face) -> np.ndarray:
    """A face image u32[H,W] as rgba8 ``[H, W, 4]``: a fixed integer hash of the index (a multiply by 2654435761 mod 2^32, xor-folded by 15 bits; the low
    three bytes, each or-ed with 0x40 so that no face is black), alpha 255; ``NO_FACE`` all zero."""
    f = np.ascontiguousarray(face, np.uint32)
    x = (f.astype(np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x ^= x >> np.uint32(15)
    out = np.stack([(x & np.uint32(0xFF)) | np.uint32(0x40), ((x >> np.uint32(8)) & np.uint32(0xFF)) | np.uint32(0x40),
                    ((x >> np.uint32(16)) & np.uint32(0xFF)) | np.uint32(0x40), np.full(f.shape, 255, np.uint32)], axis=-1).astype(np.uint8)
    out[f == np.uint32(NO_FACE)] = 0
    return out


def encodeDepthAgreement(device: HipDevice, a: HipBuffer, b: HipBuffer, width: int, height: int, maxDifference: float, threshold: float, out: HipBuffer,
                         bWeightSum: Optional[HipBuffer] = None, minWeightSum: float = 0.0) -> None:
    """Stream-ordered ``depthAgreement``: the five u64 sums into the first 40 bytes of ``out``.  No host wait."""
    n = int(width) * int(height)
    if a.size < 4 * n or b.size < 4 * n or (bWeightSum is not None and bWeightSum.size < 4 * n) or out.size < 40:
        raise ValueError(f"depthAgreement: buffers too small for {width}x{height}")
    check(device.lib.wdgs_depth_agreement(device.handle, a.ptr, b.ptr, bWeightSum.ptr if bWeightSum is not None else None, float(minWeightSum), int(width), int(height),
                                          float(maxDifference), float(threshold), out.ptr))


def _depth_agreement_result(sums, maxDifference: float) -> dict:
    both, only_a, only_b, within, sum_q = (int(x) for x in sums)
    mean = (sum_q * float(np.float32(maxDifference)) / 2.0 ** 24 / both) if both else float("nan")
    return dict(both=both, onlyA=only_a, onlyB=only_b, within=within, sum_q=sum_q, mean=mean)


def depthAgreement(device: HipDevice, a, b, width: int, height: int, maxDifference: float, threshold: float, bWeightSum=None, minWeightSum: float = 0.0) -> dict:
    """How far two f32 depth images (numpy or ``HipBuffer``) agree: ``both``, ``onlyA``, ``onlyB`` count the pixels where both, ``a`` alone, ``b`` alone
    have a depth (finite and > 0; ``b`` also only where ``bWeightSum >= minWeightSum`` when that image is given); ``within`` those of ``both`` with
    ``|a - b| <= threshold``; ``sum_q`` the sum of ``u32(min(|a - b| / maxDifference, 1) 2^24)`` and ``mean = sum_q maxDifference / 2^24 / both`` the mean
    absolute difference clamped at ``maxDifference`` (nan when ``both`` is 0).  Exact integer sums.  ``0 < threshold <= maxDifference``.  Synchronises."""
    n = int(width) * int(height)
    owned = []

    def on_device(x, what):
        if x is None or isinstance(x, HipBuffer):
            return x
        arr = np.ascontiguousarray(x, np.float32).reshape(-1)
        if arr.size != n:
            raise ValueError(f"depthAgreement: {what} has {arr.size} values for {width}x{height}")
        owned.append(device.bufferFrom(arr, f"depthAgreement: {what}"))
        return owned[-1]

    out = device.createBuffer(40, "depth agreement")
    try:
        encodeDepthAgreement(device, on_device(a, "a"), on_device(b, "b"), width, height, maxDifference, threshold, out, on_device(bWeightSum, "bWeightSum"), minWeightSum)
        return _depth_agreement_result(out.read(np.uint64, count=5), maxDifference)
    finally:
        out.destroy()
        for x in owned:
            x.destroy()


# ----------------------------------------------------------------------------- mesh accuracy metrics (no reference counterpart)
NO_INDEX = 0xFFFFFFFF
KNN_EXCLUDE_SELF = 1   # WDGS_KNN_EXCLUDE_SELF


def _as_device(device: HipDevice, array, dtype, width: int, what: str) -> tuple:
    """``(buffer, rows, owned)`` of a ``[rows, width]`` array given as numpy (uploaded; ``owned``) or as a ``HipBuffer`` (whole rows of it)."""
    if isinstance(array, HipBuffer):
        return array, array.size // (np.dtype(dtype).itemsize * width), False
    a = np.ascontiguousarray(array, dtype)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{what}: expected an array of shape [N, {width}], got {a.shape}")
    return device.bufferFrom(a, what), a.shape[0], True


class MeshSampler:
    """Area-weighted surface sampling of a triangle mesh on the device (``wdgs_mesh_sampler``): ``count`` gives every triangle its dithered share of
    ``density`` samples per unit area and returns the total, ``emit`` writes them, one thread per sample.  ``sampleMesh`` is the one-call form."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_sampler_create(device.handle, C.byref(h)))
        self.handle = h

    def count(self, vertices: HipBuffer, numVertices: int, faces: HipBuffer, numFaces: int, density: float, seed: int = 0) -> int:
        """The number of samples (count, scan; waits).  ``CapacityError`` for 2^31 or more."""
        if vertices.size < 12 * int(numVertices) or faces.size < 12 * int(numFaces):
            raise ValueError("MeshSampler.count: buffers too small for the mesh")
        n = C.c_uint64(0)
        check(self.device.lib.wdgs_mesh_sampler_count(self.handle, vertices.ptr, int(numVertices), faces.ptr, int(numFaces), float(density), int(seed) & 0xFFFFFFFF, C.byref(n)))
        return int(n.value)

    def emit(self, vertices: HipBuffer, numVertices: int, faces: HipBuffer, numFaces: int, density: float, seed: int, points: HipBuffer,
             face: Optional[HipBuffer] = None, capacity: Optional[int] = None) -> None:
        """Writes ``points`` f32[total][3] and ``face`` u32[total] (optional) for the arguments of the count before it (``StateError`` otherwise;
        ``CapacityError`` when there is too little room).  Stream-ordered."""
        cap = min(points.size // 12, face.size // 4 if face is not None else 2 ** 32 - 1) if capacity is None else int(capacity)
        if cap * 12 > points.size or (face is not None and cap * 4 > face.size):
            raise ValueError("MeshSampler.emit: the capacity exceeds the buffers")
        check(self.device.lib.wdgs_mesh_sampler_emit(self.handle, vertices.ptr, int(numVertices), faces.ptr, int(numFaces), float(density), int(seed) & 0xFFFFFFFF,
                                                     points.ptr, face.ptr if face is not None else None, cap))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_sampler_destroy(self.handle)
        self.handle = None


def sampleMesh(device: HipDevice, mesh: dict, density: float, seed: int = 0, asBuffers: bool = False) -> dict:
    """Points on the surface of ``mesh`` -- the dict ``extractMesh`` and ``loaders.loadMeshPLY`` return, or ``dict(vertices=HipBuffer, faces=HipBuffer)`` on the
    device -- ``density`` per unit area on average, every triangle getting ``floor(area density + dither)`` of them: ``dict(points f32[N,3], face u32[N])``,
    the samples of a triangle consecutive, triangles in order.  A function of its arguments alone, bit for bit (include/webdgs.h states it).
    ``asBuffers``: ``points`` and ``face`` stay on the device as ``HipBuffer`` and ``count`` is added."""
    vbuf, nv, own_v = _as_device(device, mesh["vertices"], np.float32, 3, "sampleMesh: vertices")
    fbuf, nf, own_f = _as_device(device, mesh["faces"], np.uint32, 3, "sampleMesh: faces")
    sampler = MeshSampler(device)
    points = face = None
    try:
        total = sampler.count(vbuf, nv, fbuf, nf, density, seed)
        points = device.createBuffer(12 * max(total, 1), "mesh samples")
        face = device.createBuffer(4 * max(total, 1), "mesh sample faces")
        sampler.emit(vbuf, nv, fbuf, nf, density, seed, points, face, total)
        if asBuffers:
            device.synchronize()   # (the uploaded mesh is released below)
            out = dict(points=points, face=face, count=total)
            points = face = None
            return out
        return dict(points=points.read(np.float32, count=3 * total).reshape(total, 3), face=face.read(np.uint32, count=total))
    finally:
        sampler.destroy()
        for b, own in ((vbuf, own_v), (fbuf, own_f), (points, True), (face, True)):
            if own and b is not None:
                b.destroy()


# ----------------------------------------------------------------------------- mesh connected components (no reference counterpart)
class MeshComponents:
    """Connected components of an indexed mesh on the device (``wdgs_mesh_components``): ``label`` cuts the faces into components (a lock-free
    union-find, one wait), ``select`` takes the components to keep, ``compact`` writes the kept part.  ``meshComponents`` and ``removeSmallComponents``
    are the one-call forms; include/webdgs.h states the definitions."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numFaces = self.numVertices = self.count = self.invalidFaces = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_components_create(device.handle, C.byref(h)))
        self.handle = h

    def label(self, faces: HipBuffer, numFaces: int, numVertices: int) -> int:
        """Labels ``faces`` u32[numFaces][3] over ``numVertices`` vertices and returns the number of components (waits once)."""
        if not (0 <= int(numFaces) < 2 ** 32 and 0 <= int(numVertices) < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshComponents.label: bad counts {numFaces}, {numVertices}")
        if faces is not None and int(numFaces) < 2 ** 31 and faces.size < 12 * int(numFaces):
            raise ValueError("MeshComponents.label: buffer too small for the faces")
        n, bad = C.c_uint32(0), C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_components_label(self.handle, faces.ptr if faces is not None else None, int(numFaces), int(numVertices), C.byref(n), C.byref(bad)))
        self.numFaces, self.numVertices, self.count, self.invalidFaces = int(numFaces), int(numVertices), int(n.value), int(bad.value)
        return self.count

    def read(self) -> dict:
        """The last labelling as numpy: ``dict(count, faceComponent u32[F], vertexComponent u32[V], triangles u32[C], vertices u32[C], invalidFaces)``."""
        p = [C.c_void_p() for _ in range(4)]
        check(self.device.lib.wdgs_mesh_components_get(self.handle, *[C.byref(x) for x in p]))
        sizes = (self.numFaces, self.numVertices, self.count, self.count)
        arrays = [self.device.view(x.value, 4 * n).read(np.uint32, count=n) if n else np.zeros(0, np.uint32) for x, n in zip(p, sizes)]
        return dict(count=self.count, faceComponent=arrays[0], vertexComponent=arrays[1], triangles=arrays[2], vertices=arrays[3], invalidFaces=self.invalidFaces)

    def select(self, keep) -> tuple:
        """``keep``: bool[C].  Returns ``(keptVertices, keptFaces)`` (flags, scans; waits)."""
        k = np.ascontiguousarray(np.asarray(keep).astype(bool).reshape(-1), np.uint8)
        nv, nf = C.c_uint32(0), C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_components_select(self.handle, k.ctypes.data if k.size else None, int(k.size), C.byref(nv), C.byref(nf)))
        return int(nv.value), int(nf.value)

    def compact(self, vertices: Optional[HipBuffer], verticesOut: Optional[HipBuffer], facesOut: HipBuffer, vertexMap: Optional[HipBuffer] = None,
                faceMap: Optional[HipBuffer] = None, capacityVertices: Optional[int] = None, capacityFaces: Optional[int] = None) -> None:
        """Writes the kept part for the last ``select``: ``verticesOut`` f32[V'][3] gathered from ``vertices``, ``facesOut`` u32[F'][3] renumbered,
        ``vertexMap`` u32[V'], ``faceMap`` u32[F'].  ``CapacityError``, with nothing written, when there is too little room.  Stream-ordered."""
        cv = min([b.size // s for b, s in ((verticesOut, 12), (vertexMap, 4)) if b is not None] or [2 ** 32 - 1]) if capacityVertices is None else int(capacityVertices)
        cf = min([b.size // s for b, s in ((facesOut, 12), (faceMap, 4)) if b is not None] or [2 ** 32 - 1]) if capacityFaces is None else int(capacityFaces)
        for b, s, n in ((verticesOut, 12, cv), (vertexMap, 4, cv), (facesOut, 12, cf), (faceMap, 4, cf)):
            if b is not None and n * s > b.size:
                raise ValueError("MeshComponents.compact: the capacity exceeds the buffers")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_components_compact(self.handle, ptr(vertices), ptr(verticesOut), ptr(facesOut), ptr(vertexMap), ptr(faceMap), cv, cf))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_components_destroy(self.handle)
        self.handle = None


def meshComponents(device: HipDevice, mesh: dict) -> dict:
    """The connected components of ``mesh`` -- the dict ``extractMesh`` and ``loaders.loadMeshPLY`` return, or ``dict(vertices=HipBuffer, faces=HipBuffer)``
    on the device: ``dict(count, faceComponent u32[F], vertexComponent u32[V], triangles u32[C], vertices u32[C], invalidFaces)``.  Two vertices are
    connected when a face names both (shared vertices, not shared edges: the rules differ only at pinch points of a welded mesh; a mesh with duplicated
    vertices falls apart into its triangles); components are numbered in ascending order of their lowest vertex; ``0xFFFFFFFF`` marks a face that names
    a vertex ``>= V`` and a vertex that no face names.  A function of the mesh alone, bit for bit (include/webdgs.h states it)."""
    vbuf, nv, own_v = _as_device(device, mesh["vertices"], np.float32, 3, "meshComponents: vertices")
    fbuf, nf, own_f = _as_device(device, mesh["faces"], np.uint32, 3, "meshComponents: faces")
    comp = MeshComponents(device)
    try:
        comp.label(fbuf, nf, nv)
        return comp.read()
    finally:
        comp.destroy()
        for b, own in ((vbuf, own_v), (fbuf, own_f)):
            if own:
                b.destroy()


def _is_default_selection(keepLargest, minTriangles, minFraction) -> bool:
    return keepLargest is None and not minTriangles > 0 and not minFraction > 0


def selectComponents(triangles, keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0) -> np.ndarray:
    """Which components to keep, ``bool[C]``, from their sizes: ranked by (triangles descending, component number ascending), a component is kept when it
    is among the first ``keepLargest`` (``None``: all), has ``triangles >= minTriangles`` and ``triangles >= minFraction * largest`` (the product formed
    and compared in float64).  Host side."""
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1)
    keep = np.zeros(t.size, bool)
    if t.size == 0:
        return keep
    if keepLargest is not None and int(keepLargest) < 0:
        raise ValueError("selectComponents: keepLargest must be None or >= 0")
    order = np.lexsort((np.arange(t.size), -t.astype(np.int64)))
    first = order if keepLargest is None else order[: int(keepLargest)]
    keep[first] = True
    keep &= t.astype(np.int64) >= int(minTriangles)
    keep &= t.astype(np.float64) >= np.float64(minFraction) * np.float64(t.max())
    return keep


def removeSmallComponents(device: HipDevice, mesh: dict, keepLargest: Optional[int] = None, minTriangles: int = 0, minFraction: float = 0.0,
                          asBuffers: bool = False) -> dict:
    """``mesh`` without the components ``selectComponents`` does not keep: ``dict(vertices f32[V',3], faces u32[F',3], vertexMap u32[V'], faceMap u32[F'],
    components u32[kept])`` and ``colours`` / ``keys`` gathered through ``vertexMap`` when the input has them.  Kept faces stay in their order, kept
    vertices in ascending original index (a vertex is kept exactly when its component is), faces are rewritten to the new indices; ``components`` holds
    the kept components' triangle counts in component order.  Keeping everything still drops invalid faces and unreferenced vertices; a second call
    reproduces the first.  Labelled, selected and compacted on the device (``MeshComponents``); the selection itself is the host's.
    ``asBuffers``: ``vertices``, ``faces``, ``vertexMap`` and ``faceMap`` stay on the device as ``HipBuffer`` (of at least one element's size),
    ``numVertices`` and ``numFaces`` are added, ``colours`` and ``keys`` are not gathered; the caller destroys them (``destroyBuffers``)."""
    vbuf, nv, own_v = _as_device(device, mesh["vertices"], np.float32, 3, "removeSmallComponents: vertices")
    fbuf, nf, own_f = _as_device(device, mesh["faces"], np.uint32, 3, "removeSmallComponents: faces")
    comp = MeshComponents(device)
    outs = []
    try:
        comp.label(fbuf, nf, nv)
        sizes = comp.read()["triangles"]
        keep = selectComponents(sizes, keepLargest, minTriangles, minFraction)
        kv, kf = comp.select(keep)
        outs = [device.createBuffer(s * max(n, 1), "compacted mesh") for s, n in ((12, kv), (12, kf), (4, kv), (4, kf))]
        comp.compact(vbuf, outs[0], outs[1], outs[2], outs[3], kv, kf)
        if asBuffers:
            device.synchronize()   # (an uploaded mesh is released below)
            result, outs = dict(vertices=outs[0], faces=outs[1], vertexMap=outs[2], faceMap=outs[3], numVertices=kv, numFaces=kf, components=sizes[keep]), []
            return result
        out = dict(vertices=outs[0].read(np.float32, count=3 * kv).reshape(kv, 3), faces=outs[1].read(np.uint32, count=3 * kf).reshape(kf, 3),
                   vertexMap=outs[2].read(np.uint32, count=kv), faceMap=outs[3].read(np.uint32, count=kf), components=sizes[keep])
    finally:
        comp.destroy()
        for b, own in [(vbuf, own_v), (fbuf, own_f)] + [(b, True) for b in outs]:
            if own:
                b.destroy()
    for name in ("colours", "keys"):
        if name in mesh:
            out[name] = None if mesh[name] is None else np.ascontiguousarray(np.asarray(mesh[name])[out["vertexMap"]])
    return out


# ----------------------------------------------------------------------------- per-face visibility and removal of unseen faces
VISIBILITY_STATS = ("views", "foreignPixels", "countedPixels", "agreeingPixels")


def _fraction_q16(fraction: float, what: str) -> int:
    """``rint(fraction 65536)`` for a fraction in [0, 1]: what ``wdgs_face_visibility_flags`` compares with."""
    x = float(fraction)
    if not 0.0 <= x <= 1.0:
        raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"{what}: minAgreeingFraction {fraction} is not in [0, 1]")
    return int(np.rint(np.float64(x) * 65536.0))


def _rule_counts(minPixels, minViews, minAgreeing, what: str) -> tuple:
    rule = (int(minPixels), int(minViews), int(minAgreeing))
    if not all(0 <= x < 2 ** 32 for x in rule):
        raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"{what}: minPixels, minViews, minAgreeing {rule} must fit 32 unsigned bits")
    return rule


class FaceVisibility:
    """Per-face counters over views (``wdgs_face_visibility``): ``reset`` sizes them for a mesh, ``accumulate`` adds one view -- the face image
    ``MeshRasterizer.encode`` wrote and, optionally, the mesh's and the model's depth images -- ``read`` / ``buffer`` hand out ``u32[F][3]`` =
    ``{pixels, agreeing, views}``, ``flags`` applies the rule on the device and ``stats`` reads the totals.  Integer sums: every byte is a function of
    the inputs (include/webdgs.h states the definition).  ``faceVisibility`` is the one-call form without a model."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numFaces = 0
        h = C.c_void_p()
        check(device.lib.wdgs_face_visibility_create(device.handle, C.byref(h)))
        self.handle = h

    def reset(self, numFaces: int) -> None:
        """Sizes and zeroes the counters for ``numFaces`` faces; the accumulated views start at 0.  A call that grows the arrays waits once."""
        if not 0 <= int(numFaces) < 2 ** 32:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"FaceVisibility.reset: bad face count {numFaces}")
        check(self.device.lib.wdgs_face_visibility_reset(self.handle, int(numFaces)))
        self.numFaces = int(numFaces)

    def accumulate(self, faceImage: Optional[HipBuffer], width: int, height: int, meshDepth: Optional[HipBuffer] = None, modelDepth: Optional[HipBuffer] = None,
                   modelWeightSum: Optional[HipBuffer] = None, minWeightSum: float = 0.0, threshold: float = 0.05) -> None:
        """One view of ``width`` x ``height``: ``faceImage`` u32, and both or neither of ``meshDepth`` and ``modelDepth`` f32 (``modelWeightSum`` f32
        beside them, optional).  A pixel agrees when both depths are present (``depthAgreement``'s rule) and ``|mesh - model| <= threshold``; without
        depth images every counted pixel agrees.  Stream-ordered, recordable.  ``CapacityError``, with nothing written, when one more view of this
        size could carry a pixel count past 32 bits."""
        w, h = int(width), int(height)
        if not (0 <= w < 2 ** 32 and 0 <= h < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"FaceVisibility.accumulate: bad image size {width}x{height}")
        if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE:
            for b in (faceImage, meshDepth, modelDepth, modelWeightSum):
                if b is not None and b.size < 4 * w * h:
                    raise ValueError(f"FaceVisibility.accumulate: an image is too small for {w}x{h}")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_face_visibility_accumulate(self.handle, ptr(faceImage), ptr(meshDepth), ptr(modelDepth), ptr(modelWeightSum), float(minWeightSum),
                                                              float(threshold), w, h))

    def buffer(self) -> Optional[HipBuffer]:
        """The counters ``u32[F][3]`` on the device as of this call (one launch writes them; ``None`` for no faces), valid until the next ``buffer``,
        ``read``, ``reset`` or ``destroy``.  Stream-ordered, recordable."""
        p = C.c_void_p()
        check(self.device.lib.wdgs_face_visibility_get(self.handle, C.byref(p)))
        return self.device.view(p.value, 12 * self.numFaces, "face visibility counters") if self.numFaces else None

    def read(self) -> np.ndarray:
        """The counters as numpy ``u32[F, 3]`` = ``{pixels, agreeing, views}`` (waits)."""
        b = self.buffer()
        return b.read(np.uint32, count=3 * self.numFaces).reshape(self.numFaces, 3) if b is not None else np.zeros((0, 3), np.uint32)

    def flags(self, keep: Optional[HipBuffer], minPixels: int = 1, minViews: int = 1, minAgreeing: int = 0, minAgreeingFraction: float = 0.0) -> None:
        """``keep`` u8[F] on the device from the current counters, by ``selectFaces``' rule.  Stream-ordered, recordable."""
        encodeFaceVisibilityFlags(self.device, self.buffer(), self.numFaces, keep, minPixels, minViews, minAgreeing, minAgreeingFraction)

    def stats(self) -> dict:
        """``dict(views, foreignPixels, countedPixels, agreeingPixels)`` since the reset (waits)."""
        v = [C.c_uint64(0) for _ in VISIBILITY_STATS]
        check(self.device.lib.wdgs_face_visibility_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(VISIBILITY_STATS, (int(x.value) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_face_visibility_destroy(self.handle)
        self.handle = None


def encodeFaceVisibilityFlags(device: HipDevice, counters: Optional[HipBuffer], numFaces: int, keep: Optional[HipBuffer], minPixels: int = 1, minViews: int = 1,
                              minAgreeing: int = 0, minAgreeingFraction: float = 0.0) -> None:
    """``wdgs_face_visibility_flags``: ``keep`` u8[numFaces] from ``counters`` u32[numFaces][3], both on the device.  Stream-ordered, recordable."""
    n = int(numFaces)
    if not 0 <= n < 2 ** 32:
        raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"faceVisibilityFlags: bad face count {numFaces}")
    rule = _rule_counts(minPixels, minViews, minAgreeing, "faceVisibilityFlags")
    q16 = _fraction_q16(minAgreeingFraction, "faceVisibilityFlags")
    if n < 2 ** 31 and ((counters is not None and counters.size < 12 * n) or (keep is not None and keep.size < n)):
        raise ValueError("faceVisibilityFlags: buffers too small for the faces")
    ptr = lambda b: b.ptr if b is not None else None
    check(device.lib.wdgs_face_visibility_flags(device.handle, ptr(counters), n, *rule, q16, ptr(keep)))


def selectFaces(counters, minPixels: int = 1, minViews: int = 1, minAgreeing: int = 0, minAgreeingFraction: float = 0.0) -> np.ndarray:
    """Which faces to keep, ``bool[F]``, from ``counters`` u32[F, 3] = ``{pixels, agreeing, views}``: ``pixels >= minPixels``, ``views >= minViews``,
    ``agreeing >= minAgreeing`` and ``agreeing 65536 >= rint(minAgreeingFraction 65536) pixels`` in 64-bit integers.  The host restatement of
    ``FaceVisibility.flags``, bit for bit."""
    c = np.ascontiguousarray(counters, np.uint32).reshape(-1, 3).astype(np.uint64)
    rule = _rule_counts(minPixels, minViews, minAgreeing, "selectFaces")
    q16 = np.uint64(_fraction_q16(minAgreeingFraction, "selectFaces"))
    return ((c[:, 0] >= np.uint64(rule[0])) & (c[:, 2] >= np.uint64(rule[1])) & (c[:, 1] >= np.uint64(rule[2]))
            & (c[:, 1] * np.uint64(65536) >= q16 * c[:, 0]))


class MeshFaceFilter:
    """``MeshComponents``' compaction for an arbitrary face mask (``wdgs_mesh_face_filter``): ``select`` takes the faces and a u8 flag per face on the
    device, ``compact`` writes the kept part.  ``filterFaces`` is the one-call form."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_face_filter_create(device.handle, C.byref(h)))
        self.handle = h

    def select(self, faces: Optional[HipBuffer], numFaces: int, numVertices: int, keep: Optional[HipBuffer]) -> tuple:
        """``(keptVertices, keptFaces, invalidFaces)`` for ``faces`` u32[numFaces][3] over ``numVertices`` vertices under ``keep`` u8[numFaces]: a face
        is kept when its flag is non-zero and its indices are vertices, a vertex exactly when a kept face names it (flags, scans; waits)."""
        nf, nv = int(numFaces), int(numVertices)
        if not (0 <= nf < 2 ** 32 and 0 <= nv < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshFaceFilter.select: bad counts {numFaces}, {numVertices}")
        if nf < 2 ** 31 and ((faces is not None and faces.size < 12 * nf) or (keep is not None and keep.size < nf)):
            raise ValueError("MeshFaceFilter.select: buffers too small for the faces")
        ptr = lambda b: b.ptr if b is not None else None
        kv, kf, bad = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_face_filter_select(self.handle, ptr(faces), nf, nv, ptr(keep), C.byref(kv), C.byref(kf), C.byref(bad)))
        return int(kv.value), int(kf.value), int(bad.value)

    def compact(self, vertices: Optional[HipBuffer], verticesOut: Optional[HipBuffer], facesOut: Optional[HipBuffer], vertexMap: Optional[HipBuffer] = None,
                faceMap: Optional[HipBuffer] = None, capacityVertices: Optional[int] = None, capacityFaces: Optional[int] = None) -> None:
        """``MeshComponents.compact``'s arguments and rules for the last ``select``.  Stream-ordered, recordable."""
        cv = min([b.size // s for b, s in ((verticesOut, 12), (vertexMap, 4)) if b is not None] or [2 ** 32 - 1]) if capacityVertices is None else int(capacityVertices)
        cf = min([b.size // s for b, s in ((facesOut, 12), (faceMap, 4)) if b is not None] or [2 ** 32 - 1]) if capacityFaces is None else int(capacityFaces)
        for b, s, n in ((verticesOut, 12, cv), (vertexMap, 4, cv), (facesOut, 12, cf), (faceMap, 4, cf)):
            if b is not None and n * s > b.size:
                raise ValueError("MeshFaceFilter.compact: the capacity exceeds the buffers")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_face_filter_compact(self.handle, ptr(vertices), ptr(verticesOut), ptr(facesOut), ptr(vertexMap), ptr(faceMap), cv, cf))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_face_filter_destroy(self.handle)
        self.handle = None


def filterFaces(device: HipDevice, mesh: dict, keep, asBuffers: bool = False) -> dict:
    """``mesh`` without the faces whose ``keep`` flag (``bool[F]`` / ``u8[F]`` numpy, or a u8[F] ``HipBuffer``) is zero, and without the vertices no kept
    face names: ``dict(vertices f32[V',3], faces u32[F',3], vertexMap u32[V'], faceMap u32[F'], invalidFaces)`` and ``colours`` / ``keys`` gathered
    through ``vertexMap`` when the input has them -- ``removeSmallComponents``' shape and rules (kept faces in their order, kept vertices in ascending
    original index; a face that names no vertex is never kept).  ``mesh``: numpy, or a dict of ``HipBuffer`` as ``_mesh_on_device`` takes (left as it
    is).  ``asBuffers``: the four arrays stay on the device as ``HipBuffer`` (of at least one element's size), ``numVertices`` and ``numFaces`` are
    added, ``colours`` and ``keys`` are not gathered; the caller destroys them (``destroyBuffers``)."""
    vbuf, fbuf, nv, nf, own = _mesh_on_device(device, mesh, "filterFaces")
    kbuf, own_k = keep, False
    filt = None
    outs = []
    try:
        if not isinstance(keep, HipBuffer):
            k = np.ascontiguousarray(np.asarray(keep).astype(bool).reshape(-1), np.uint8)
            if k.size != nf:
                raise ValueError(f"filterFaces: {k.size} flags for {nf} faces")
            kbuf, own_k = device.bufferFrom(k, "filterFaces: flags"), True
        filt = MeshFaceFilter(device)
        kv, kf, bad = filt.select(fbuf, nf, nv, kbuf)
        outs = [device.createBuffer(s * max(n, 1), "filtered mesh") for s, n in ((12, kv), (12, kf), (4, kv), (4, kf))]
        filt.compact(vbuf, outs[0], outs[1], outs[2], outs[3], kv, kf)
        if asBuffers:
            device.synchronize()   # (an uploaded mesh is released below)
            result, outs = dict(vertices=outs[0], faces=outs[1], vertexMap=outs[2], faceMap=outs[3], numVertices=kv, numFaces=kf, invalidFaces=bad), []
            return result
        out = dict(vertices=outs[0].read(np.float32, count=3 * kv).reshape(kv, 3), faces=outs[1].read(np.uint32, count=3 * kf).reshape(kf, 3),
                   vertexMap=outs[2].read(np.uint32, count=kv), faceMap=outs[3].read(np.uint32, count=kf), invalidFaces=bad)
    finally:
        if filt is not None:
            filt.destroy()
        for b, o in [(vbuf, own), (fbuf, own), (kbuf, own_k)] + [(b, True) for b in outs]:
            if o:
                b.destroy()
    for name in ("colours", "keys"):
        if name in mesh and not isinstance(mesh[name], HipBuffer):
            out[name] = None if mesh[name] is None else np.ascontiguousarray(np.asarray(mesh[name])[out["vertexMap"]])
    return out


def faceVisibility(device: HipDevice, mesh: dict, cameras, width: int, height: int, near: float = MESH_RASTER_NEAR, cull: str = "none") -> dict:
    """Which faces of ``mesh`` the ``cameras`` (68-float blocks, numpy or ``HipBuffer``) see, without a model: every camera's face image is rasterized at
    ``width`` x ``height`` and accumulated.  ``dict(counters u32[F,3] = {pixels, agreeing, views}, stats)`` -- ``agreeing`` equals ``pixels`` here, and
    ``stats`` is ``FaceVisibility.stats``'s dict.  ``selectFaces`` and ``filterFaces`` take it from there."""
    w, h = int(width), int(height)
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, "faceVisibility")
    rasterizer = visibility = image = None
    try:
        rasterizer, visibility = MeshRasterizer(device), FaceVisibility(device)
        visibility.reset(F)
        npix = w * h if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE else 0
        image = device.createBuffer(4 * max(npix, 1), "mesh face image")
        for camera in cameras:
            cam, own_cam = _camera_on_device(device, camera, "faceVisibility")
            try:
                rasterizer.encode(vertices, V, faces, F, None, cam, w, h, near, cull, face=image)
                visibility.accumulate(image, w, h)
            finally:
                if own_cam:
                    device.synchronize()
                    cam.destroy()
        return dict(counters=visibility.read(), stats=visibility.stats())
    finally:
        for o in (visibility, rasterizer, image):
            if o is not None:
                o.destroy()
        if own:
            vertices.destroy()
            faces.destroy()


# ----------------------------------------------------------------------------- vertex colours baked from photographs
BAKE_STATS = ("usable", "inImage", "visible", "accumulated", "viewportMismatch", "bakedVertices")


class MeshColourBaker:
    """Per-vertex colour sums over views (``wdgs_mesh_colour_baker``): ``reset`` sizes them for a mesh, ``accumulate`` adds one view -- a photograph, its
    camera block and, optionally, the vertex normals (the weights) and the depth image ``MeshRasterizer.encode`` wrote for this mesh and camera (the
    occlusion test) -- ``resolve`` turns the sums into rgba8 vertex colours, ``read`` hands out the sums and ``stats`` the totals.  Integer sums: the
    state does not depend on the order of the views and every byte is a function of the inputs (include/webdgs.h states the definition).
    ``bakeVertexColours`` is the one-call form."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numVertices = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_colour_baker_create(device.handle, C.byref(h)))
        self.handle = h

    def reset(self, numVertices: int) -> None:
        """Sizes and zeroes the state for ``numVertices`` vertices.  A call that grows the arrays waits once; it cannot be recorded."""
        if not 0 <= int(numVertices) < 2 ** 32:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshColourBaker.reset: bad vertex count {numVertices}")
        check(self.device.lib.wdgs_mesh_colour_baker_reset(self.handle, int(numVertices)))
        self.numVertices = int(numVertices)

    def accumulate(self, vertices: Optional[HipBuffer], numVertices: int, camera: HipBuffer, image: Optional[HipBuffer], width: int, height: int,
                   normals: Optional[HipBuffer] = None, meshDepth: Optional[HipBuffer] = None, near: float = MESH_RASTER_NEAR, depthTolerance: float = 0.05,
                   minCos: float = 0.1) -> None:
        """One view of ``width`` x ``height``: ``vertices`` f32[numVertices][3], the 68-float ``camera`` block, ``image`` rgba8, and optionally ``normals``
        f32[numVertices][3] and ``meshDepth`` f32.  A vertex is coloured by this view when it projects into the image, all four depth texels round it
        are within ``depthTolerance`` of its own depth, and the cosine between its normal and the direction to the camera is at least ``minCos``; the
        view's weight is that cosine.  Stream-ordered, recordable."""
        nv, w, h = int(numVertices), int(width), int(height)
        if not (0 <= nv < 2 ** 32 and 0 <= w < 2 ** 32 and 0 <= h < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshColourBaker.accumulate: bad counts {numVertices}, {width}x{height}")
        if nv < 2 ** 31 and any(b is not None and b.size < 12 * nv for b in (vertices, normals)):
            raise ValueError("MeshColourBaker.accumulate: buffers too small for the vertices")
        if camera is not None and camera.size < 272:
            raise ValueError("MeshColourBaker.accumulate: the camera block has 68 floats")
        if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE:
            for b in (image, meshDepth):
                if b is not None and b.size < 4 * w * h:
                    raise ValueError(f"MeshColourBaker.accumulate: an image is too small for {w}x{h}")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_colour_baker_accumulate(self.handle, ptr(vertices), ptr(normals), nv, ptr(camera), ptr(image), ptr(meshDepth), w, h, float(near),
                                                                float(depthTolerance), float(minCos)))

    def resolve(self, coloursOut: Optional[HipBuffer], numVertices: int, fallback: Optional[HipBuffer] = None, bakedOut: Optional[HipBuffer] = None,
                minViews: int = 1, minWeight: int = 1) -> None:
        """``coloursOut`` rgba8[numVertices] from the current sums: a vertex at least ``minViews`` views coloured with a weight sum of at least
        ``minWeight`` (a view adds at most 256) gets its weighted mean, alpha 255; any other ``fallback``'s colour (which may be ``coloursOut``
        itself), or zeros.  ``bakedOut`` u8[numVertices]: which.  Stream-ordered, recordable."""
        nv = int(numVertices)
        if not (0 <= nv < 2 ** 32 and 0 <= int(minViews) < 2 ** 32 and 0 <= int(minWeight) < 2 ** 64):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshColourBaker.resolve: bad counts {numVertices}, {minViews}, {minWeight}")
        if nv < 2 ** 31 and (any(b is not None and b.size < 4 * nv for b in (coloursOut, fallback)) or (bakedOut is not None and bakedOut.size < nv)):
            raise ValueError("MeshColourBaker.resolve: buffers too small for the vertices")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_colour_baker_resolve(self.handle, ptr(coloursOut), ptr(fallback), ptr(bakedOut), nv, int(minViews), int(minWeight)))

    def read(self) -> tuple:
        """``(sums u64[V, 4] = {R, G, B, Wt}, views u32[V])`` as numpy (waits)."""
        sums, views = np.zeros((self.numVertices, 4), np.uint64), np.zeros(self.numVertices, np.uint32)
        check(self.device.lib.wdgs_mesh_colour_baker_read(self.handle, sums.ctypes.data, views.ctypes.data))
        return sums, views

    def stats(self) -> dict:
        """``dict(usable, inImage, visible, accumulated, viewportMismatch, bakedVertices)``: the vertices that passed each step summed over the views
        since the reset, the calls whose camera block was of another image size, and the baked vertices of the last resolve (waits)."""
        v = [C.c_uint64(0) for _ in BAKE_STATS]
        check(self.device.lib.wdgs_mesh_colour_baker_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(BAKE_STATS, (int(x.value) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_colour_baker_destroy(self.handle)
        self.handle = None


def _bake_views(device: HipDevice, vertices: HipBuffer, faces: HipBuffer, V: int, F: int, normals: Optional[HipBuffer], fallback: Optional[HipBuffer], views: list,
                depthTolerance: float, minCos: float, minViews: int, minWeight: int, near: float, occlusion: bool) -> tuple:
    """``(colours, baked, stats)``: new rgba8[V] and u8[V] buffers -- the caller destroys them -- of a mesh on the device baked from ``views``, a list of
    ``(camera, image, width, height)`` on the device.  The rasterizer is grown once, to the largest view, before the loop; per view one encode (with
    ``occlusion``) and one accumulate; then one resolve."""
    sizes = [(int(w), int(h)) for _, _, w, h in views]
    legal = [(w, h) for w, h in sizes if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE]
    baker = rasterizer = depth = None
    out = {}
    try:
        baker = MeshColourBaker(device)
        baker.reset(V)
        if occlusion and legal:
            w, h = max(legal, key=lambda s: s[0] * s[1])
            depth = device.createBuffer(4 * w * h, "mesh depth")
            rasterizer = MeshRasterizer(device)
            rasterizer.encode(vertices, V, faces, F, None, views[sizes.index((w, h))][0], w, h, near, "none", depth=depth)
        for (camera, image, _, _), (w, h) in zip(views, sizes):
            if rasterizer is not None and (w, h) in legal:
                rasterizer.encode(vertices, V, faces, F, None, camera, w, h, near, "none", depth=depth)
            baker.accumulate(vertices, V, camera, image, w, h, normals, depth if occlusion else None, near, depthTolerance, minCos)
        out = dict(colours=device.createBuffer(4 * max(V, 1), "baked colours"), baked=device.createBuffer(max(V, 1), "baked mask"))
        baker.resolve(out["colours"], V, fallback, out["baked"], minViews, minWeight)
        stats = baker.stats()   # (waits: the objects released below are idle)
        result, out = (out["colours"], out["baked"], stats), {}
        return result
    finally:
        for o in (baker, rasterizer, depth):
            if o is not None:
                o.destroy()
        destroyBuffers(out)


def bakeMeshFromViews(device: HipDevice, mesh: dict, views: list, normals: bool = True, depthTolerance: float = 0.05, minCos: float = 0.1, minViews: int = 1,
                      minWeight: int = 1, near: float = MESH_RASTER_NEAR, occlusion: bool = True, asBuffers: bool = False, what: str = "bakeVertexColours") -> dict:
    """``bakeVertexColours`` for views that are on the device already: ``views`` is a list of ``(camera, image, width, height)`` with ``HipBuffer``s, which
    may differ in size (``Evaluator.bakeMeshColours`` hands in the trainer's own cameras and photographs)."""
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, what)
    owned = [vertices, faces] if own else []
    try:
        fallback, own_fallback = _mesh_colours_on_device(device, mesh, V, own, what)
        if own_fallback:
            owned.append(fallback)
        nbuf = None
        if normals:
            n = mesh.get("normals")
            if isinstance(n, HipBuffer):
                nbuf = n
            elif n is not None:
                n = np.ascontiguousarray(n, np.float32)
                if n.shape != (V, 3):
                    raise ValueError(f"{what}: normals of shape {n.shape} for {V} vertices")
                nbuf = device.bufferFrom(n, f"{what}: normals")
                owned.append(nbuf)
            else:
                _, nbuf, _ = _smooth_and_normals(device, vertices, faces, V, F, None, True)
                owned.append(nbuf)
        colours, baked, stats = _bake_views(device, vertices, faces, V, F, nbuf, fallback, views, depthTolerance, minCos, minViews, minWeight, near, occlusion)
        if asBuffers:
            return dict(mesh, colours=colours, baked=baked, stats=stats)
        try:
            rgba = colours.read(np.uint8, count=4 * V).reshape(V, 4)
            return dict(mesh, colours=np.ascontiguousarray(rgba[:, :3]), baked=baked.read(np.uint8, count=V).astype(bool), stats=stats)
        finally:
            colours.destroy()
            baked.destroy()
    finally:
        device.synchronize()
        for b in owned:
            b.destroy()


def bakeVertexColours(device: HipDevice, mesh: dict, cameras, images, width: int, height: int, normals: bool = True, depthTolerance: float = 0.05, minCos: float = 0.1,
                      minViews: int = 1, minWeight: int = 1, near: float = MESH_RASTER_NEAR, occlusion: bool = True, asBuffers: bool = False) -> dict:
    """``mesh`` with its vertex colours taken from photographs, without a model: per ``camera`` (68-float blocks, numpy or ``HipBuffer``) and its ``image``
    (rgba8 ``[height, width, 4]`` numpy, or a ``HipBuffer``) the mesh's depth image is rasterized (``occlusion``) and every vertex that projects into the
    photograph, is not hidden (all four depth texels round it within ``depthTolerance`` of its own depth) and faces the camera adds the bilinear sample
    there, weighted by the cosine between its normal and the direction to the camera.  A vertex at least ``minViews`` views coloured, with a weight sum
    of at least ``minWeight`` (256 per view that looks straight at it), gets the weighted mean; any other keeps the mesh's own colour (zeros for a mesh
    without colours).

    ``mesh``: numpy, or a dict of ``HipBuffer`` as ``_mesh_on_device`` takes (left as it is).  ``normals=True``: the weights use the mesh's ``normals``,
    computed by ``vertexNormals``' kernels when it carries none; ``False``: every view weighs the same and back-facing views are not excluded.
    ``minCos`` = 0.1 is a caller's knob, not a tuned number: it only keeps grazing views, whose samples are smeared along the surface, out of the mean.
    Returns the mesh dict with ``colours`` u8[V, 3] replaced -- what ``loaders.saveMeshPLY`` writes -- and ``baked`` bool[V] and ``stats``
    (``MeshColourBaker.stats``) added; ``asBuffers``: ``colours`` rgba8[V] (alpha 255 where baked) and ``baked`` u8[V] stay on the device as ``HipBuffer``
    the caller destroys.  A function of its arguments alone, bit for bit."""
    cameras, images = list(cameras), list(images)
    if len(cameras) != len(images):
        raise ValueError(f"bakeVertexColours: {len(cameras)} cameras for {len(images)} images")
    w, h = int(width), int(height)
    owned, views = [], []
    try:
        for camera, image in zip(cameras, images):
            cam, own_cam = _camera_on_device(device, camera, "bakeVertexColours")
            if own_cam:
                owned.append(cam)
            if not isinstance(image, HipBuffer):
                a = np.ascontiguousarray(image, np.uint8)
                if a.size != 4 * w * h:
                    raise ValueError(f"bakeVertexColours: an image of shape {a.shape} for {w}x{h} rgba8")
                image = device.bufferFrom(a, "bakeVertexColours: image")
                owned.append(image)
            views.append((cam, image, w, h))
        return bakeMeshFromViews(device, mesh, views, normals, depthTolerance, minCos, minViews, minWeight, near, occlusion, asBuffers)
    finally:
        device.synchronize()
        for b in owned:
            b.destroy()


# ----------------------------------------------------------------------------- a texture atlas baked from photographs
TEXTURE_STATS = ("invalidFaces", "facingAwayFaces", "offImageFaces", "usable", "inImage", "visible", "accumulated", "viewportMismatch", "bakedTexels",
                 "filledTexels", "fallbackTexels")
TEXTURE_CELLS = (4, 8, 16, 32)


def textureLayout(numFaces: int, cell: int = 8) -> dict:
    """The atlas of ``numFaces`` faces in square cells of ``cell`` texels, two faces per cell (include/webdgs.h states it): ``dict(width, height, cellsPerRow,
    uv f32[F, 3, 2])`` with the per-corner texture coordinates in the OBJ convention -- ``u = (x + 0.5) / width``, ``v = 1 - (y + 0.5) / height`` for the
    atlas texel ``(x, y)`` a corner sits on, computed in doubles and rounded once.  Arithmetic in ``(numFaces, cell)`` alone; no device work."""
    F, c = int(numFaces), int(cell)
    if not 0 <= F < 2 ** 31:
        raise ValueError(f"textureLayout: {numFaces} faces (0 to 2^31 - 1)")
    if c not in TEXTURE_CELLS:
        raise ValueError(f"textureLayout: a cell of {cell} texels (4, 8, 16 or 32)")
    cells = (F + 1) // 2
    per_row = math.isqrt(cells)
    if per_row * per_row < cells:
        per_row += 1
    rows = -(-cells // per_row) if per_row else 0
    width, height = per_row * c, rows * c
    if width > _lib.MESH_TEXTURE_MAX_SIZE:
        raise ValueError(f"textureLayout: {F} faces in cells of {c} texels need an atlas {width} texels wide (at most {_lib.MESH_TEXTURE_MAX_SIZE})")
    m = c - 3
    f = np.arange(F, dtype=np.int64)
    k, odd = f // 2, (f % 2)[:, None, None]
    corner = np.array([[0, 0], [m, 0], [0, m]], np.int64)[None]          # (i', j') of v0, v1, v2
    local = np.where(odd == 1, c - 1 - corner, corner)                    # (i, j) in the cell: the odd face's chart is turned by 180 degrees
    x = ((k % max(per_row, 1)) * c)[:, None] + local[:, :, 0]
    y = ((k // max(per_row, 1)) * c)[:, None] + local[:, :, 1]
    uv = np.stack([(x + 0.5) / max(width, 1), 1.0 - (y + 0.5) / max(height, 1)], axis=2).astype(np.float32)
    return dict(width=width, height=height, cellsPerRow=per_row, uv=uv)


class MeshTextureBaker:
    """Per-texel colour sums of a mesh's texture atlas over views (``wdgs_mesh_texture_baker``): ``reset`` lays the atlas out for a face count and a cell
    size and zeroes the sums, ``accumulate`` adds one view -- a photograph, its camera block and, optionally, the depth image ``MeshRasterizer.encode`` wrote
    for this mesh and camera (the occlusion test) -- ``resolve`` turns the sums into an rgba8 texture, ``read`` hands out the sums and ``stats`` the totals.
    Integer sums: the state does not depend on the order of the views and every byte is a function of the inputs (include/webdgs.h states the
    definition).  ``bakeTexture`` is the one-call form."""

    def __init__(self, device: HipDevice):
        self.device = device
        self.destroyed = False
        self.numFaces = self.cell = self.width = self.height = self.cellsPerRow = 0
        h = C.c_void_p()
        check(device.lib.wdgs_mesh_texture_baker_create(device.handle, C.byref(h)))
        self.handle = h

    def reset(self, numFaces: int, cell: int = 8, _accumulates: int = 0) -> dict:
        """Lays the atlas out and zeroes the state; returns ``layout()``.  A call that grows the array waits once; it cannot be recorded.  ``_accumulates``
        is where the count of views starts, for the test of the refusal of the 65536th."""
        if not (0 <= int(numFaces) < 2 ** 32 and 0 <= int(cell) < 2 ** 32 and 0 <= int(_accumulates) < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshTextureBaker.reset: bad counts {numFaces}, {cell}, {_accumulates}")
        check(self.device.lib.wdgs_mesh_texture_baker_reset(self.handle, int(numFaces), int(cell), int(_accumulates)))
        self.numFaces, self.cell = int(numFaces), int(cell)
        return self.layout()

    def layout(self) -> dict:
        """``dict(width, height, cellsPerRow)`` of the last reset (``textureLayout`` gives the same, and the texture coordinates)."""
        w, h, r = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.device.lib.wdgs_mesh_texture_baker_layout(self.handle, C.byref(w), C.byref(h), C.byref(r)))
        self.width, self.height, self.cellsPerRow = int(w.value), int(h.value), int(r.value)
        return dict(width=self.width, height=self.height, cellsPerRow=self.cellsPerRow)

    def accumulate(self, vertices: Optional[HipBuffer], numVertices: int, faces: Optional[HipBuffer], numFaces: int, camera: HipBuffer, image: Optional[HipBuffer],
                   width: int, height: int, meshDepth: Optional[HipBuffer] = None, near: float = MESH_RASTER_NEAR, depthTolerance: float = 0.05, minCos: float = 0.1,
                   twoSided: bool = False) -> None:
        """One view of ``width`` x ``height``.  A texel is coloured by this view when its point on the face projects into the image, all four depth texels
        round it are within ``depthTolerance`` of its own depth, and the cosine between the face's normal and the direction to the camera is at least
        ``minCos``; the view's weight is that cosine.  Stream-ordered, recordable."""
        nv, nf, w, h = int(numVertices), int(numFaces), int(width), int(height)
        if not (0 <= nv < 2 ** 32 and 0 <= nf < 2 ** 32 and 0 <= w < 2 ** 32 and 0 <= h < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshTextureBaker.accumulate: bad counts {numVertices}, {numFaces}, {width}x{height}")
        if (nv < 2 ** 31 and vertices is not None and vertices.size < 12 * nv) or (nf < 2 ** 31 and faces is not None and faces.size < 12 * nf):
            raise ValueError("MeshTextureBaker.accumulate: buffers too small for the mesh")
        if camera is not None and camera.size < 272:
            raise ValueError("MeshTextureBaker.accumulate: the camera block has 68 floats")
        if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE:
            for b in (image, meshDepth):
                if b is not None and b.size < 4 * w * h:
                    raise ValueError(f"MeshTextureBaker.accumulate: an image is too small for {w}x{h}")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_texture_baker_accumulate(self.handle, ptr(vertices), nv, ptr(faces), nf, ptr(camera), ptr(image), ptr(meshDepth), w, h, float(near),
                                                                 float(depthTolerance), float(minCos), 1 if twoSided else 0))

    def resolve(self, faces: Optional[HipBuffer], numFaces: int, numVertices: int, textureOut: Optional[HipBuffer], colours: Optional[HipBuffer] = None,
                stateOut: Optional[HipBuffer] = None, minWeight: int = 1, fill: bool = True) -> None:
        """``textureOut`` rgba8[height][width] from the current sums: a texel with a weight sum of at least ``minWeight`` (a view adds at most 256) gets its
        weighted mean; with ``fill`` any other texel next to such texels of its own face gets their mean; the rest the mesh's vertex ``colours``
        rgba8[numVertices] (zeros without) interpolated over the face.  ``stateOut`` u8[height][width]: 1 baked, 2 filled, 0 otherwise.  Stream-ordered,
        recordable."""
        nf, nv = int(numFaces), int(numVertices)
        if not (0 <= nf < 2 ** 32 and 0 <= nv < 2 ** 32 and 0 <= int(minWeight) < 2 ** 32):
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"MeshTextureBaker.resolve: bad counts {numFaces}, {numVertices}, {minWeight}")
        n = self.width * self.height
        if (textureOut is not None and textureOut.size < 4 * n) or (stateOut is not None and stateOut.size < n):
            raise ValueError(f"MeshTextureBaker.resolve: an output is too small for {self.width}x{self.height}")
        if (nf < 2 ** 31 and faces is not None and faces.size < 12 * nf) or (nv < 2 ** 31 and colours is not None and colours.size < 4 * nv):
            raise ValueError("MeshTextureBaker.resolve: buffers too small for the mesh")
        ptr = lambda b: b.ptr if b is not None else None
        check(self.device.lib.wdgs_mesh_texture_baker_resolve(self.handle, ptr(faces), nf, nv, ptr(colours), ptr(textureOut), ptr(stateOut), int(minWeight), 1 if fill else 0))

    def read(self) -> np.ndarray:
        """The sums ``u32[cells * cell * cell, 4] = {R, G, B, Wsum}``, cell-major: texel ``(i, j)`` of cell ``k`` is row ``k cell^2 + j cell + i`` (waits)."""
        rows = np.zeros((((self.numFaces + 1) // 2) * self.cell * self.cell, 4), np.uint32)
        check(self.device.lib.wdgs_mesh_texture_baker_read(self.handle, rows.ctypes.data))
        return rows

    def stats(self) -> dict:
        """``TEXTURE_STATS``: the faces each face-level test stopped and the texels that passed each step, summed over the views since the reset; the calls
        whose camera block was of another image size; the baked, filled and fallback texels of the last resolve (waits)."""
        v = (C.c_uint64 * len(TEXTURE_STATS))()
        check(self.device.lib.wdgs_mesh_texture_baker_stats(self.handle, v))
        return dict(zip(TEXTURE_STATS, (int(x) for x in v)))

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_mesh_texture_baker_destroy(self.handle)
        self.handle = None


def bakeTextureFromViews(device: HipDevice, mesh: dict, views: list, cell: int = 8, depthTolerance: float = 0.05, minCos: float = 0.1, minWeight: int = 1,
                         near: float = MESH_RASTER_NEAR, occlusion: bool = True, twoSided: bool = False, fill: bool = True, asBuffers: bool = False,
                         what: str = "bakeTexture") -> dict:
    """``bakeTexture`` for views that are on the device already: ``views`` is a list of ``(camera, image, width, height)`` with ``HipBuffer``s, which may
    differ in size.  As ``bakeMeshFromViews`` does, the rasterizer is grown once, to the largest view, before the loop; per view one encode (with
    ``occlusion``) and one accumulate; then one resolve."""
    vertices, faces, V, F, own = _mesh_on_device(device, mesh, what)
    owned = [vertices, faces] if own else []
    baker = rasterizer = depth = None
    out = {}
    try:
        colours, own_colours = _mesh_colours_on_device(device, mesh, V, own, what)
        if own_colours:
            owned.append(colours)
        layout = textureLayout(F, cell)
        sizes = [(int(w), int(h)) for _, _, w, h in views]
        legal = [(w, h) for w, h in sizes if 1 <= w <= _lib.MESH_RASTER_MAX_SIZE and 1 <= h <= _lib.MESH_RASTER_MAX_SIZE]
        baker = MeshTextureBaker(device)
        baker.reset(F, cell)
        if occlusion and legal:
            w, h = max(legal, key=lambda s: s[0] * s[1])
            depth = device.createBuffer(4 * w * h, "mesh depth")
            rasterizer = MeshRasterizer(device)
            rasterizer.encode(vertices, V, faces, F, None, views[sizes.index((w, h))][0], w, h, near, "none", depth=depth)
        for (camera, image, _, _), (w, h) in zip(views, sizes):
            if rasterizer is not None and (w, h) in legal:
                rasterizer.encode(vertices, V, faces, F, None, camera, w, h, near, "none", depth=depth)
            baker.accumulate(vertices, V, faces, F, camera, image, w, h, depth if occlusion else None, near, depthTolerance, minCos, twoSided)
        Wt, Ht = layout["width"], layout["height"]
        out = dict(texture=device.createBuffer(4 * max(Wt * Ht, 1), "baked texture"), texelState=device.createBuffer(max(Wt * Ht, 1), "texel state"))
        baker.resolve(faces, F, V, out["texture"], colours, out["texelState"], minWeight, fill)
        stats = baker.stats()   # (waits: the objects released below are idle)
        extra = dict(uv=layout["uv"], textureWidth=Wt, textureHeight=Ht, textureCell=int(cell), textureStats=stats)
        if asBuffers:
            result, out = dict(mesh, **out, **extra), {}
            return result
        return dict(mesh, texture=out["texture"].read(np.uint8, count=4 * Wt * Ht).reshape(Ht, Wt, 4),
                    texelState=out["texelState"].read(np.uint8, count=Wt * Ht).reshape(Ht, Wt), **extra)
    finally:
        device.synchronize()
        for o in (baker, rasterizer, depth):
            if o is not None:
                o.destroy()
        destroyBuffers(out)
        for b in owned:
            b.destroy()


def bakeTexture(device: HipDevice, mesh: dict, cameras, images, width: int, height: int, cell: int = 8, depthTolerance: float = 0.05, minCos: float = 0.1,
                minWeight: int = 1, near: float = MESH_RASTER_NEAR, occlusion: bool = True, twoSided: bool = False, fill: bool = True, asBuffers: bool = False) -> dict:
    """``mesh`` with a texture atlas taken from photographs, without a model.  Every face gets its own small chart -- two faces share a square cell of
    ``cell`` texels (4, 8, 16 or 32), ``textureLayout`` -- so the detail the photographs hold between two vertices survives ``simplifyMesh``.  Per ``camera``
    (68-float blocks, numpy or ``HipBuffer``) and its ``image`` (rgba8 ``[height, width, 4]`` numpy, or a ``HipBuffer``) the mesh's depth image is
    rasterized (``occlusion``) and every texel whose point on its face projects into the photograph, is not hidden and faces the camera (``twoSided``:
    either way) adds the bilinear sample there, weighted by the cosine between the face's normal and the direction to the camera.  A texel with a weight
    sum of at least ``minWeight`` (256 per view that looks straight at it) gets the weighted mean; with ``fill`` an unseen texel next to seen ones of its
    face gets their mean; any other the mesh's vertex colours interpolated (zeros for a mesh without colours).

    Returns the mesh dict with ``texture`` u8[Ht, Wt, 4] (row 0 at the top; texels no face owns are zero), ``uv`` f32[F, 3, 2] per face corner (the OBJ
    convention: ``loaders.saveMeshOBJ`` writes both), ``texelState`` u8[Ht, Wt] (1 baked, 2 filled, 0 otherwise), ``textureWidth``, ``textureHeight``,
    ``textureCell`` and ``textureStats`` (``MeshTextureBaker.stats``) added; ``asBuffers``: ``texture`` and ``texelState`` stay on the device as
    ``HipBuffer`` the caller destroys.  A function of its arguments alone, bit for bit."""
    cameras, images = list(cameras), list(images)
    if len(cameras) != len(images):
        raise ValueError(f"bakeTexture: {len(cameras)} cameras for {len(images)} images")
    w, h = int(width), int(height)
    owned, views = [], []
    try:
        for camera, image in zip(cameras, images):
            cam, own_cam = _camera_on_device(device, camera, "bakeTexture")
            if own_cam:
                owned.append(cam)
            if not isinstance(image, HipBuffer):
                a = np.ascontiguousarray(image, np.uint8)
                if a.size != 4 * w * h:
                    raise ValueError(f"bakeTexture: an image of shape {a.shape} for {w}x{h} rgba8")
                image = device.bufferFrom(a, "bakeTexture: image")
                owned.append(image)
            views.append((cam, image, w, h))
        return bakeTextureFromViews(device, mesh, views, cell, depthTolerance, minCos, minWeight, near, occlusion, twoSided, fill, asBuffers)
    finally:
        device.synchronize()
        for b in owned:
            b.destroy()


class PointIndex:
    """A uniform grid over ``points`` ([M,3] float32 as numpy, or a ``HipBuffer``) for exact nearest-point queries under a cutoff (``wdgs_point_index``).
    ``cellSize`` is a speed parameter only -- no result depends on it; ``None``: chosen by the first query (its cutoff, or less for many points), which then
    finishes the build.  Non-finite
    points are left out.  The build waits once (it reads the points' bounds back); queries are stream-ordered."""

    def __init__(self, device: HipDevice, points, cellSize: Optional[float] = None, count: Optional[int] = None):
        self.device = device
        self.destroyed = False
        self._points, n, self._owned = _as_device(device, points, np.float32, 3, "PointIndex: points")
        self.numPoints = n if count is None else int(count)
        if self.numPoints > n:
            raise ValueError("PointIndex: the count exceeds the buffer")
        h = C.c_void_p()
        check(device.lib.wdgs_point_index_create(device.handle, self._points.ptr, self.numPoints, 0.0 if cellSize is None else float(cellSize), C.byref(h)))
        self.handle = h

    def info(self) -> dict:
        """``dict(cellSize, dims, indexed)``: the cell edge in use (0 before the first query of an index made without one), the grid, the finite points."""
        c, d, n = C.c_float(0), (C.c_uint32 * 3)(), C.c_uint32(0)
        check(self.device.lib.wdgs_point_index_info(self.handle, C.byref(c), d, C.byref(n)))
        return dict(cellSize=float(c.value), dims=tuple(int(x) for x in d), indexed=int(n.value))

    def reserveQueries(self, count: int) -> None:
        """Room for queries of ``count`` points: what a recorded ``nearestInto`` needs beforehand (an eager query makes its own)."""
        check(self.device.lib.wdgs_point_index_reserve_queries(self.handle, int(count)))

    def nearestInto(self, encoder: Optional[HipEncoder], queries: HipBuffer, count: int, maxDistance: float, d2: HipBuffer, index: HipBuffer,
                    pairs: Optional[HipBuffer] = None) -> None:
        """Stream-ordered ``nearest``: for the first ``count`` points of ``queries`` the squared distance (f32, in f32 arithmetic) to the nearest indexed point
        within ``maxDistance`` into ``d2`` and that point's index into ``index`` -- the lowest index among equally near ones; ``+inf`` and ``0xFFFFFFFF`` when there
        is none or the query is not finite.  ``pairs`` (optional, 8 bytes): the number of pairs examined is added to it.  No host wait; records."""
        k = int(count)
        if queries.size < 12 * k or d2.size < 4 * k or index.size < 4 * k or (pairs is not None and pairs.size < 8):
            raise ValueError(f"PointIndex.nearest: buffers too small for {k} queries")
        check(self.device.lib.wdgs_point_index_nearest(self.handle, queries.ptr, k, float(maxDistance), d2.ptr, index.ptr, pairs.ptr if pairs is not None else None))

    def nearest(self, queries, maxDistance: float) -> dict:
        """``dict(d2 f32[K], index u32[K])`` for ``queries`` ([K,3] numpy or a ``HipBuffer``).  Synchronises."""
        qbuf, k, owned = _as_device(self.device, queries, np.float32, 3, "PointIndex.nearest: queries")
        d2 = self.device.createBuffer(4 * max(k, 1), "nearest d2")
        index = self.device.createBuffer(4 * max(k, 1), "nearest index")
        try:
            self.nearestInto(None, qbuf, k, maxDistance, d2, index)
            return dict(d2=d2.read(np.float32, count=k), index=index.read(np.uint32, count=k))
        finally:
            d2.destroy()
            index.destroy()
            if owned:
                qbuf.destroy()

    def bounds(self) -> dict:
        """``dict(lo, hi)``: the bounding box of the finite points (f32[3] each; zeros when there is none).  No device work."""
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        check(self.device.lib.wdgs_point_index_bounds(self.handle, lo, hi))
        return dict(lo=np.array(lo, np.float32), hi=np.array(hi, np.float32))

    def kNearestInto(self, encoder: Optional[HipEncoder], queries: HipBuffer, count: int, k: int, maxDistance: float, d2: HipBuffer, index: HipBuffer,
                     excludeSelf: bool = False, pairs: Optional[HipBuffer] = None) -> None:
        """Stream-ordered ``kNearest``: for each of the first ``count`` points of ``queries`` the ``k`` (1 to 16) nearest indexed points within ``maxDistance``,
        ordered by (squared distance, index), into row ``i`` of ``d2`` f32[count, k] and ``index`` u32[count, k]; slots beyond the candidates, and every slot of
        a non-finite query, hold ``+inf`` and ``0xFFFFFFFF``.  ``excludeSelf``: query ``i`` leaves out the indexed point ``i`` (the self-query, where the
        queries are the indexed points).  ``pairs`` (optional, 8 bytes): the number of pairs examined is added to it.  No host wait; records."""
        n, kk = int(count), int(k)
        if kk < 0 or kk > 0xFFFFFFFF:
            raise ValueError(f"PointIndex.kNearest: k = {k}")
        if queries.size < 12 * n or d2.size < 4 * n * kk or index.size < 4 * n * kk or (pairs is not None and pairs.size < 8):
            raise ValueError(f"PointIndex.kNearest: buffers too small for {n} queries with k = {kk}")
        check(self.device.lib.wdgs_point_index_k_nearest(self.handle, queries.ptr, n, kk, float(maxDistance), KNN_EXCLUDE_SELF if excludeSelf else 0, d2.ptr, index.ptr,
                                                         pairs.ptr if pairs is not None else None))

    def kNearest(self, queries, k: int, maxDistance: float, excludeSelf: bool = False) -> dict:
        """``dict(d2 f32[K, k], index u32[K, k])`` for ``queries`` ([K,3] numpy or a ``HipBuffer``).  Synchronises."""
        qbuf, n, owned = _as_device(self.device, queries, np.float32, 3, "PointIndex.kNearest: queries")
        kk = int(k)
        slots = n * max(0, min(kk, 1024))   # (the library refuses a k outside [1, 16])
        d2 = self.device.createBuffer(4 * max(slots, 1), "kNearest d2")
        index = self.device.createBuffer(4 * max(slots, 1), "kNearest index")
        try:
            self.kNearestInto(None, qbuf, n, kk, maxDistance, d2, index, excludeSelf)
            return dict(d2=d2.read(np.float32, count=n * kk).reshape(n, kk), index=index.read(np.uint32, count=n * kk).reshape(n, kk))
        finally:
            d2.destroy()
            index.destroy()
            if owned:
                qbuf.destroy()

    def destroy(self) -> None:
        if self.destroyed:
            return
        self.destroyed = True
        self.device.lib.wdgs_point_index_destroy(self.handle)
        self.handle = None
        if self._owned:
            self._points.destroy()
        self._points = None


def initScalesFromNeighbours(device: HipDevice, pointCloud, k: int = 3, maxDistance: Optional[float] = None, minD2: float = 1e-7, count: Optional[int] = None) -> dict:
    """3DGS's scale initialisation, in place: every point of ``pointCloud`` gets ``log sigma = 0.5 log(max(mean, minD2))`` on all three axes, ``mean`` the
    mean squared distance to its ``k`` nearest other points within ``maxDistance`` (fewer when fewer are there; a point without any keeps its scales).  The
    distances are those of the records' fp16 positions, which is what the renderer sees.  ``maxDistance=None``: twice the widest extent of the finite
    positions, so every other finite point is a candidate -- for a cloud with far outliers pass a cutoff instead.  Only halves 8, 9, 10
    of each record of ``gaussian_3d_buffer`` change.  Returns ``dict(meanD2 f32[N], found u32[N])``: ``mean`` (``+inf`` without a neighbour) and the number
    of neighbours it was taken over.  Synchronises."""
    n = int(pointCloud.num_points) if count is None else int(count)
    if n < 0 or n > int(pointCloud.num_points):
        raise ValueError("initScalesFromNeighbours: the count exceeds the point cloud")
    if pointCloud.gaussian_3d_buffer.size < 24 * n:
        raise ValueError("initScalesFromNeighbours: the Gaussian buffer is too small for the count")
    kk = int(k)
    lib, g = device.lib, pointCloud.gaussian_3d_buffer
    slots = n * max(0, min(kk, 1024))   # (the library refuses a k outside [1, 16])
    positions = device.createBuffer(12 * max(n, 1), "neighbour positions")
    d2 = device.createBuffer(4 * max(slots, 1), "neighbour d2")
    idx = device.createBuffer(4 * max(slots, 1), "neighbour index")
    mean = device.createBuffer(4 * max(n, 1), "neighbour mean d2")
    index = None
    try:
        check(lib.wdgs_point_cloud_positions(device.handle, g.ptr, n, positions.ptr))
        index = PointIndex(device, positions, count=n)
        if maxDistance is None:
            b = index.bounds()
            widest = float(np.max(b["hi"].astype(np.float64) - b["lo"].astype(np.float64)))
            maxDistance = 2.0 * widest if widest > 0.0 else 1.0
        index.kNearestInto(None, positions, n, kk, maxDistance, d2, idx, excludeSelf=True)
        check(lib.wdgs_point_cloud_neighbour_scales(device.handle, g.ptr, n, d2.ptr, kk, float(minD2), mean.ptr))
        found = np.isfinite(d2.read(np.float32, count=n * kk).reshape(n, kk)).sum(axis=1).astype(np.uint32)
        return dict(meanD2=mean.read(np.float32, count=n), found=found)
    finally:
        if index is not None:
            index.destroy()
        for b in (positions, d2, idx, mean):
            b.destroy()


def encodePointDistanceStats(device: HipDevice, d2: HipBuffer, count: int, maxDistance: float, threshold: float, out: HipBuffer) -> None:
    """Stream-ordered ``pointDistanceStats``: the three u64 sums into the first 24 bytes of ``out``.  No host wait."""
    if d2.size < 4 * int(count) or out.size < 24:
        raise ValueError(f"pointDistanceStats: buffers too small for {count} distances")
    check(device.lib.wdgs_point_distance_stats(device.handle, d2.ptr, int(count), float(maxDistance), float(threshold), out.ptr))


def pointDistanceStats(device: HipDevice, d2, maxDistance: float, threshold: float, count: Optional[int] = None) -> dict:
    """Exact integer statistics of ``PointIndex.nearest``'s squared distances (numpy, or a ``HipBuffer`` with ``count``): ``n`` of them, ``n_found`` finite,
    ``n_within`` with ``d2 <= threshold^2``, ``sum_q`` the sum of ``u32(sqrt(d2) / maxDistance 2^24)`` over the found, and ``mean = sum_q maxDistance / 2^24 /
    n_found`` (nan when nothing was found).  ``0 < threshold <= maxDistance``.  Synchronises."""
    if isinstance(d2, HipBuffer):
        buf, n, owned = d2, (d2.size // 4 if count is None else int(count)), False
    else:
        a = np.ascontiguousarray(d2, np.float32).reshape(-1)
        buf, n, owned = device.bufferFrom(a, "d2"), a.size, True
    out = device.createBuffer(24, "distance stats")
    try:
        encodePointDistanceStats(device, buf, n, maxDistance, threshold, out)
        found, within, sum_q = (int(x) for x in out.read(np.uint64, count=3))
    finally:
        out.destroy()
        if owned:
            buf.destroy()
    mean = (sum_q * float(np.float32(maxDistance)) / 2.0 ** 24 / found) if found else float("nan")
    return dict(n=n, n_found=found, n_within=within, sum_q=sum_q, mean=mean)


def geometryMetrics(device: HipDevice, points, reference, maxDistance: float, threshold: float) -> dict:
    """How far a point set is from a reference set, in both directions (the DTU and Tanks-and-Temples numbers): ``accuracy`` the mean distance from ``points``
    to their nearest ``reference`` point, over the points that have one within ``maxDistance`` (the others are outliers: counted, not averaged),
    ``completeness`` the same from the reference to the points, ``chamfer`` their mean, ``precision`` / ``recall`` the share of points / reference points within
    ``threshold``, ``fscore = 2PR / (P + R)`` (0 when both are 0); a direction with nothing found gives nan.  Both sets: [N,3] float32 numpy or ``HipBuffer``."""
    pbuf, np_, own_p = _as_device(device, points, np.float32, 3, "geometryMetrics: points")
    rbuf, nr, own_r = _as_device(device, reference, np.float32, 3, "geometryMetrics: reference")
    d2 = device.createBuffer(4 * max(np_, nr, 1), "metrics d2")
    idx = device.createBuffer(4 * max(np_, nr, 1), "metrics index")
    out = device.createBuffer(48, "metrics sums")
    indices = []
    try:
        for k, (src, n_src, dst, n_dst) in enumerate(((pbuf, np_, rbuf, nr), (rbuf, nr, pbuf, np_))):
            index = PointIndex(device, dst, count=n_dst)
            indices.append(index)
            index.nearestInto(None, src, n_src, maxDistance, d2, idx)
            check(device.lib.wdgs_point_distance_stats(device.handle, d2.ptr, n_src, float(maxDistance), float(threshold), out.ptr + 24 * k))
        s = [int(x) for x in out.read(np.uint64, count=6)]
    finally:
        for index in indices:
            index.destroy()
        for b, own in ((d2, True), (idx, True), (out, True), (pbuf, own_p), (rbuf, own_r)):
            if own:
                b.destroy()
    scale = float(np.float32(maxDistance)) / 2.0 ** 24
    acc = s[2] * scale / s[0] if s[0] else float("nan")
    comp = s[5] * scale / s[3] if s[3] else float("nan")
    p = s[1] / np_ if np_ else float("nan")
    r = s[4] / nr if nr else float("nan")
    return dict(accuracy=acc, completeness=comp, chamfer=(acc + comp) / 2, precision=p, recall=r, fscore=0.0 if (p == 0 and r == 0) else 2 * p * r / (p + r),
                n_points=np_, n_reference=nr, outliers_points=np_ - s[0], outliers_reference=nr - s[3])


# ----------------------------------------------------------------------------- per-Gaussian contribution (no reference counterpart)
CONTRIBUTION_RECORD_BYTES = 16
CONTRIBUTION_DTYPE = np.dtype([("sum_q", "<u8"), ("max_bits", "<u4"), ("pixels", "<u4")])


def createContributionBuffer(device: HipDevice, numPoints: int) -> HipBuffer:
    """One zeroed 16-byte record ``{u64 sum_q; u32 max_bits; u32 pixels}`` per Gaussian, for ``TiledRasterizer.encodeContribution``."""
    buf = device.createBuffer(CONTRIBUTION_RECORD_BYTES * max(1, int(numPoints)), label="contribution")
    buf.clear()
    return buf


def readContribution(buffer: HipBuffer, n: int) -> dict:
    """The first ``n`` records: ``sum_q`` uint64, ``weight_sum`` float64 (``sum_q * 2^-24``), ``max_weight`` float32, ``pixels`` uint32."""
    rec = buffer.read(np.uint8, CONTRIBUTION_RECORD_BYTES * int(n)).view(CONTRIBUTION_DTYPE)
    sum_q = np.ascontiguousarray(rec["sum_q"])
    return dict(sum_q=sum_q, weight_sum=sum_q.astype(np.float64) * 2.0 ** -24, max_weight=np.ascontiguousarray(rec["max_bits"]).view(np.float32),
                pixels=np.ascontiguousarray(rec["pixels"]))


def encodeImageSSE(device: HipDevice, a: HipBuffer, b: HipBuffer, num_pixels: int, out: HipBuffer) -> None:
    """Stream-ordered ``imageSSE``: the u64 sum into the first 8 bytes of ``out``.  No host wait."""
    check(device.lib.wdgs_image_sse_rgb8(device.handle, a.ptr, b.ptr, int(num_pixels), out.ptr))


def imageSSE(device: HipDevice, a: HipBuffer, b: HipBuffer, num_pixels: int) -> int:
    """Exact sum of squared rgb8 differences of two rgba8 images (synchronises)."""
    out = device.createBuffer(8, "sse")
    check(device.lib.wdgs_image_sse_rgb8(device.handle, a.ptr, b.ptr, int(num_pixels), out.ptr))
    return int(out.read(np.uint64, count=1)[0])


def imagePSNR(device: HipDevice, a: HipBuffer, b: HipBuffer, num_pixels: int) -> float:
    """PSNR in dB over the rgb channels of two rgba8 images; +inf when identical."""
    sse = imageSSE(device, a, b, num_pixels)
    return float("inf") if sse == 0 else 10.0 * float(np.log10(255.0 * 255.0 * 3.0 * num_pixels / sse))


def psnrFromSSE(sse: int, num_pixels: int) -> float:
    """PSNR in dB of an rgb8 sum of squared differences over ``num_pixels`` pixels; +inf for 0."""
    return float("inf") if int(sse) == 0 else 10.0 * float(np.log10(255.0 * 255.0 * 3.0 * num_pixels / int(sse)))


def encodeImageSSIM(device: HipDevice, a: HipBuffer, b: HipBuffer, width: int, height: int, out: HipBuffer, map: Optional[HipBuffer] = None) -> None:
    """Stream-ordered SSIM (``wdgs_image_ssim_rgb8``): the f64 mean into the first 8 bytes of ``out``, the per-pixel, per-channel map (W*H*3 f32,
    ``map[(y*W + x)*3 + c]``) into ``map`` when given.  No host wait."""
    n = int(width) * int(height)
    if a.size < 4 * n or b.size < 4 * n or out.size < 8 or (map is not None and map.size < 12 * n):
        raise ValueError(f"encodeImageSSIM: buffers too small for {width}x{height}")
    check(device.lib.wdgs_image_ssim_rgb8(device.handle, a.ptr, b.ptr, int(width), int(height), out.ptr, map.ptr if map is not None else None))


def imageSSIM(device: HipDevice, a: HipBuffer, b: HipBuffer, width: int, height: int, map: Optional[HipBuffer] = None) -> float:
    """SSIM of two rgba8 images over their rgb channels (11x11 Gaussian window, sigma 1.5, zero padding: the 3DGS convention); 1.0 when
    identical.  ``map``: optional W*H*3 f32 buffer for the per-pixel, per-channel values.  Synchronises.  No reference counterpart."""
    out = device.createBuffer(8, "ssim")
    encodeImageSSIM(device, a, b, width, height, out, map)
    return float(out.read(np.float64, count=1)[0])


# ----------------------------------------------------------------------------- Optimizer
DEFAULT_ADAM_HYPERPARAMETERS = dict(lr_pos=0.00016, lr_color=0.0025, lr_opacity=0.05, lr_scale=0.005, lr_rot=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8)
_STATE_FIELDS = ("optPosBuffer", "optRotBuffer", "optScaleBuffer", "optOpacityBuffer", "paramSH", "stateSH")


def allocateOptimizerStateBuffers(device: HipDevice, numPoints: int) -> dict:
    """``allocateOptimizerStateBuffers`` (``src/renderers/optimizer.ts:27-38``): zero-filled."""
    sizes = (C.c_size_t * 6)()
    check(device.lib.wdgs_optimizer_state_sizes(int(numPoints), C.byref(sizes)))
    return {k: device.createBuffer(sizes[i], k) for i, k in enumerate(_STATE_FIELDS)}


def _state_struct(buffers: dict) -> _lib.OptimizerState:
    return _lib.OptimizerState(*[buffers[k].ptr for k in _STATE_FIELDS])


class Optimizer:
    """``Optimizer`` (``src/renderers/optimizer.ts:40-363``)."""

    def __init__(self, device: HipDevice, pointCloud: PointCloud, params: Optional[dict] = None, initialState: Optional[dict] = None):
        self.device, self.numPoints = device, pointCloud.num_points
        self.params = {**DEFAULT_ADAM_HYPERPARAMETERS, **(params or {})}
        self.destroyed = False
        hp = _lib.AdamHyperparameters(*[float(self.params[k]) for k in DEFAULT_ADAM_HYPERPARAMETERS])
        if initialState and initialState.get("buffers"):
            self.buffers = initialState["buffers"]  # adopted (optimizer.ts:81-88)
            it = int(initialState.get("iteration") or 0)
            fresh = False
        else:
            self.buffers = allocateOptimizerStateBuffers(device, self.numPoints)
            it, fresh = 0, True
        st = _state_struct(self.buffers)
        h = C.c_void_p()
        check(device.lib.wdgs_optimizer_create(device.handle, self.numPoints, C.byref(hp), None, None, C.byref(st), 0, it, C.byref(h)))
        self.handle = h
        self._deferred_cloud: Optional[PointCloud] = None
        if fresh:  # initBuffers (optimizer.ts:145-253): K20 unpack into the zero-filled state
            check(device.lib.wdgs_optimizer_init_from_point_cloud(h, pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr))

    def getIteration(self) -> int:
        return int(self.device.lib.wdgs_optimizer_get_iteration(self.handle))

    def getHyperparameters(self) -> dict:
        return dict(self.params)

    def setHyperparameters(self, next_params: dict) -> None:
        self.params.update(next_params)
        hp = _lib.AdamHyperparameters(*[float(self.params[k]) for k in DEFAULT_ADAM_HYPERPARAMETERS])
        check(self.device.lib.wdgs_optimizer_set_hyperparameters(self.handle, C.byref(hp)))

    def getStateBuffers(self) -> dict:
        """``getStateBuffers`` (``optimizer.ts:267-278``).  Goes through ``wdgs_optimizer_get_state`` so the compact SH-DC copy the
        kernels train is written back into ``paramSH`` / ``stateSH`` (stream-ordered) before anyone reads them."""
        st = _lib.OptimizerState()
        check(self.device.lib.wdgs_optimizer_get_state(self.handle, C.byref(st)))
        # position, log-scale and SH-DC {param, m, v} are trained in a compact copy: a handle the host keeps across steps is brought up to date
        # whenever its content is read (the reference's GPUBuffers are live)
        for b in self.buffers.values():
            if b.before_read is None:
                b.before_read = self._flush_state
        return self.buffers

    def _flush_state(self) -> None:
        if not self.destroyed and self.handle:
            st = _lib.OptimizerState()
            check(self.device.lib.wdgs_optimizer_get_state(self.handle, C.byref(st)))

    # ---- deferred SH writes (include/webdgs.h: wdgs_optimizer_set_deferred_sh; no reference counterpart)
    def setDeferredSH(self, pointCloud: PointCloud, enabled: bool = True) -> Optional[HipBuffer]:
        """On: the steps write the trained SH-DC halves to a compact array instead of the cloud's 96-byte rows; returns that array (give it
        to every forward pass that renders the cloud: ``TiledForwardPass.setDcSource``).  The cloud's SH buffer is brought up to date
        by ``flushSH`` -- automatically before any host read of it (``HipBuffer.before_read``), explicitly before device-side readers
        that have no dc source (a viewer's own forward pass, ``DensifyPrunePass.encodeScatter``).  Off: flushes and restores the
        reference's write pattern."""
        check(self.device.lib.wdgs_optimizer_set_deferred_sh(self.handle, pointCloud.sh_buffer.ptr, 1 if enabled else 0))
        self._deferred_cloud = pointCloud if enabled else None
        pointCloud.sh_buffer.before_read = (lambda: self.flushSH(pointCloud)) if enabled else None
        ptr = self.device.lib.wdgs_optimizer_dc_words(self.handle)
        words = self.device.view(ptr, 8 * max(1, self.numPoints), "sh-dc words") if (enabled and ptr) else None
        pointCloud.dc_words = words
        return words

    def flushSH(self, pointCloud: PointCloud) -> None:
        """Writes the deferred SH-DC halves into the cloud's rows (a no-op when nothing was trained since the last flush)."""
        if not self.destroyed and self.handle:
            check(self.device.lib.wdgs_optimizer_flush_sh(self.handle, pointCloud.sh_buffer.ptr))

    def applyRepackedRows(self, rows: HipBuffer, skipFirst: int, skipCount: int, guard: Optional[HipBuffer], pointCloud: PointCloud) -> None:
        """``applyRepackedRows`` for this optimizer's replica: with deferred SH writes the gathered halves go to the compact array."""
        check(self.device.lib.wdgs_optimizer_apply_repacked_rows(self.handle, rows.ptr, int(skipFirst), int(skipCount), guard.ptr if guard is not None else None,
                                                                 pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr))

    def advanceIteration(self, count: int = 1) -> None:
        """Bumps the host-side step counter when a recorded command buffer containing ``step`` is re-submitted."""
        check(self.device.lib.wdgs_optimizer_advance_iteration(self.handle, int(count)))

    def step(self, encoder, coefficients: PointCloud, gradientsBuffer: HipBuffer, tileCountsBuffer: HipBuffer) -> None:
        check(self.device.lib.wdgs_optimizer_step(self.handle, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, gradientsBuffer.ptr, tileCountsBuffer.ptr))

    def stepWithGeometry(self, encoder, coefficients: PointCloud, backwardPass: "TiledBackwardPass", cameraBuffer: HipBuffer, tileCountsBuffer: HipBuffer) -> None:
        """``step`` fused with K17 (``wdgs_optimizer_step_with_geometry``): call after ``backwardPass.encodeRaster`` for the view.  One
        pass over the Gaussians: geometry backward (the packed gradient still lands in the pass's gradient buffer), Adam, re-pack."""
        check(self.device.lib.wdgs_optimizer_step_with_geometry(self.handle, backwardPass.handle, cameraBuffer.ptr, coefficients.gaussian_3d_buffer.ptr,
                                                                coefficients.sh_buffer.ptr, tileCountsBuffer.ptr))

    def stepF32(self, encoder, coefficients: PointCloud, gradF32: HipBuffer, visibleCounts: HipBuffer) -> None:
        """Data-parallel step on fp32 gradients summed over views."""
        check(self.device.lib.wdgs_optimizer_step_f32(self.handle, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, gradF32.ptr, visibleCounts.ptr))

    def stepF32Range(self, encoder, coefficients: PointCloud, gradF32: HipBuffer, visibleCounts: HipBuffer, first: int, count: int,
                     rowsOut: Optional[HipBuffer] = None) -> None:
        """Adam + re-pack on Gaussians ``[first, first + count)`` -- the slice this rank owns after the reduce-scatter; ``rowsOut``
        also receives the re-packed 32-byte rows for the all-gather."""
        check(self.device.lib.wdgs_optimizer_step_f32_range(self.handle, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, gradF32.ptr,
                                                            visibleCounts.ptr, int(first), int(count), rowsOut.ptr if rowsOut is not None else None))

    def setGuard(self, flagBuffer: Optional[HipBuffer], offset: int = 0) -> None:
        """While the u32 at ``flagBuffer + offset`` is non-zero at execution time, ``step*`` leave every buffer untouched."""
        check(self.device.lib.wdgs_optimizer_set_guard(self.handle, (flagBuffer.ptr + offset) if flagBuffer is not None else None))

    def stateChanged(self) -> None:
        """The state arrays were rewritten from outside (slices gathered from other ranks): refresh internal copies."""
        check(self.device.lib.wdgs_optimizer_state_changed(self.handle))

    def destroy(self) -> None:
        if self.destroyed:
            return
        pc = self._deferred_cloud
        if pc is not None and self.device.handle and not pc.sh_buffer.destroyed:  # the cloud outlives its optimizer: leave its SH rows current
            try:
                self.setDeferredSH(pc, False)
            except _lib.WdgsError:
                pc.sh_buffer.before_read = None
        self.destroyed = True
        self.device.lib.wdgs_optimizer_destroy(self.handle)
        self.handle = None


def accumulateGradients(device: HipDevice, numPoints: int, gradientsBuffer: HipBuffer, tileCountsBuffer: HipBuffer, accF32: HipBuffer, visibleCounts: HipBuffer) -> None:
    check(device.lib.wdgs_accumulate_gradients(device.handle, int(numPoints), gradientsBuffer.ptr, tileCountsBuffer.ptr, accF32.ptr, visibleCounts.ptr))


def storeGradients(device: HipDevice, numPoints: int, gradientsBuffer: HipBuffer, tileCountsBuffer: HipBuffer, accF32: HipBuffer, visibleCounts: HipBuffer) -> None:
    """Overwrite form of ``accumulateGradients`` for the first view of a batch (no clearing pass needed before it)."""
    check(device.lib.wdgs_store_gradients(device.handle, int(numPoints), gradientsBuffer.ptr, tileCountsBuffer.ptr, accF32.ptr, visibleCounts.ptr))


def guardAccumulate(device: HipDevice, flag: HipBuffer, src: HipBuffer, srcOffset: int = 0, overwrite: bool = False) -> None:
    """``flag = (overwrite ? 0 : flag) | (src != 0)``: folds per-view overflow words into the guard word of a batched step."""
    check(device.lib.wdgs_guard_accumulate(device.handle, flag.ptr, src.ptr + srcOffset, 1 if overwrite else 0))


def _ptr_array(values) -> "C.Array":
    vals = [v.value if isinstance(v, C.c_void_p) else int(v) for v in values]
    return (C.c_void_p * len(vals))(*vals)


def projectViews(forwardPasses: list, cameraBuffers: list, pointCloud: PointCloud) -> None:
    """K1 of ALL the views of a batched step in one launch (``wdgs_tiled_forward_project_views``): Gaussian and SH row are read once and
    projected under every camera into that view's own forward pass.  Follow with ``forwardPasses[v].encodeProjected(encoder)``."""
    dev = forwardPasses[0].device
    for f in forwardPasses:
        f.syncDcSource()
    check(dev.lib.wdgs_tiled_forward_project_views(_ptr_array([f.handle for f in forwardPasses]), _ptr_array([c.ptr for c in cameraBuffers]), len(forwardPasses),
                                                   pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr))


def geometryViews(backwardPasses: list, cameraBuffers: list, forwardPasses: list, sums: HipBuffer, visible: HipBuffer, guard: HipBuffer, pointCloud: PointCloud,
                  writeGradients: bool = False, continues: bool = False) -> None:
    """K17 of ALL the views of a batched step in one launch (``wdgs_tiled_backward_encode_geometry_views``): what ``encodeGeometry(camera,
    accumulate=dict(first=(v == 0), ...))`` per view produces -- the step's fp32 gradient block, visibility counts and guard word -- bit for
    bit, with the Gaussians read once and the block written once.  ``continues``: these views follow earlier ones of the same step that
    were handed over in a previous call (groups, in view order)."""
    dev = backwardPasses[0].device
    counts = [f.getResources()["tileCountsBuffer"].ptr for f in forwardPasses]
    stats = [f.getStatsBuffer().ptr + 8 for f in forwardPasses]   # the overflow word of each view's stats block
    check(dev.lib.wdgs_tiled_backward_encode_geometry_views(_ptr_array([b.handle for b in backwardPasses]), _ptr_array([c.ptr for c in cameraBuffers]), _ptr_array(counts),
                                                            _ptr_array(stats), len(backwardPasses), pointCloud.gaussian_3d_buffer.ptr, sums.ptr, visible.ptr, guard.ptr,
                                                            1 if writeGradients else 0, 1 if continues else 0))


def applyRepackedRows(device: HipDevice, numPoints: int, rows: HipBuffer, skipFirst: int, skipCount: int, guard: Optional[HipBuffer],
                      pointCloud: PointCloud) -> None:
    """Writes the rows the other ranks published (all-gather) into this replica's point cloud, skipping the own slice."""
    check(device.lib.wdgs_apply_repacked_rows(device.handle, int(numPoints), rows.ptr, int(skipFirst), int(skipCount), guard.ptr if guard is not None else None,
                                              pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr))


# ----------------------------------------------------------------------------- DensifyPrunePass
class DensifyPrunePass:
    """``DensifyPrunePass`` (``src/renderers/densify-prune.ts:75-687``), strategy ``gpu_rebuild``."""

    def __init__(self, device: HipDevice, config: Optional[dict] = None):
        self.device = device
        self.config = dict(strategy="cpu_rebuild", numViews=1, cloneThreshold=0, splitThreshold=0, pruneThreshold=0, maxNewPointsPerStep=0,
                           maxBufferBytes=128 * 1024 * 1024)
        self.config.update(config or {})
        self.numPoints = 0
        c = self._cfg()
        h = C.c_void_p()
        check(device.lib.wdgs_densify_prune_create(device.handle, C.byref(c), C.byref(h)))
        self.handle = h

    def _cfg(self) -> _lib.DensifyConfig:
        c = self.config
        return _lib.DensifyConfig(max(1, int(c.get("numViews") or 1)), max(0, int(c.get("cloneThreshold") or 0)),
                                  float(c["splitThreshold"] if c.get("splitThreshold") is not None else 1e9), float(c.get("pruneThreshold") or 0.0),
                                  max(0, int(c.get("maxNewPointsPerStep") or 0)), int(c.get("maxBufferBytes") or 0))

    def setConfig(self, next_cfg: dict) -> None:
        self.config.update(next_cfg)
        c = self._cfg()
        check(self.device.lib.wdgs_densify_prune_set_config(self.handle, C.byref(c)))

    def getConfig(self) -> dict:
        return dict(self.config)

    def ensureSize(self, numPoints: int) -> None:
        check(self.device.lib.wdgs_densify_prune_ensure_size(self.handle, int(numPoints)))
        self.numPoints = int(numPoints)

    def encodePrepare(self, encoder, inputs: dict) -> dict:
        pc: PointCloud = inputs["pointCloud"]
        mc = inputs.get("metricCountsBuffer")
        out = _lib.DensifyPrepared()
        check(self.device.lib.wdgs_densify_prune_encode_prepare(self.handle, pc.num_points, pc.gaussian_3d_buffer.ptr, mc.ptr if mc is not None else None, C.byref(out)))
        self.numPoints = pc.num_points
        n, d = max(1, pc.num_points), self.device
        return dict(actionBuffer=d.view(out.action_buffer, 4 * n), outCountBuffer=d.view(out.out_count_buffer, 4 * n),
                    outOffsetBuffer=d.view(out.out_offset_buffer, 4 * n), outTotalBuffer=d.view(out.out_total_buffer, 4), maxOutPoints=int(out.max_out_points))

    # ---- the stages encodePrepare is made of (densify-prune.ts:327-456), for hosts that sequence them themselves
    def _buffers(self) -> dict:
        out = _lib.DensifyPrepared()
        check(self.device.lib.wdgs_densify_prune_get_buffers(self.handle, C.byref(out)))
        n, d = max(1, self.numPoints), self.device
        return dict(actionBuffer=d.view(out.action_buffer, 4 * n), outCountBuffer=d.view(out.out_count_buffer, 4 * n),
                    outOffsetBuffer=d.view(out.out_offset_buffer, 4 * n), outTotalBuffer=d.view(out.out_total_buffer, 4), maxOutPoints=int(out.max_out_points))

    def computeMaxOutPoints(self, pointCloud: PointCloud) -> int:
        m = C.c_uint32(0)
        check(self.device.lib.wdgs_densify_prune_compute_max_out_points(self.handle, pointCloud.num_points, C.byref(m)))
        return int(m.value)

    def encodeDecision(self, encoder, inputs: dict) -> dict:
        pc: PointCloud = inputs["pointCloud"]
        mc = inputs.get("metricCountsBuffer")
        check(self.device.lib.wdgs_densify_prune_encode_decision(self.handle, pc.num_points, pc.gaussian_3d_buffer.ptr, mc.ptr if mc is not None else None))
        self.numPoints = pc.num_points
        b = self._buffers()
        return dict(actionBuffer=b["actionBuffer"], outCountBuffer=b["outCountBuffer"])

    def encodeContributionDecision(self, encoder, numPoints: int, statsBuffer: HipBuffer, rule: dict) -> dict:
        """The decision of contribution-based pruning (no reference counterpart): a Gaussian is kept iff its record in
        ``statsBuffer`` meets every non-zero field of ``rule`` (``minMaxWeight``, ``minWeightSum``, ``minPixels``, ``minSumQ``).  Then ``encodePrefixSum``,
        ``encodeTotalOut``, ``readTotal`` and ``encodeScatter`` compact the cloud; what this stage keeps is copied bit for bit."""
        unknown = set(rule) - {"minMaxWeight", "minWeightSum", "minPixels", "minSumQ"}
        if unknown:
            raise ValueError(f"encodeContributionDecision: unknown rule fields {sorted(unknown)}")
        n = int(numPoints)
        if statsBuffer.size < CONTRIBUTION_RECORD_BYTES * n:
            raise ValueError(f"encodeContributionDecision: the statistics buffer holds {statsBuffer.size} bytes, {n} Gaussians need {CONTRIBUTION_RECORD_BYTES * n}")
        r = _lib.ContributionRule(float(rule.get("minMaxWeight") or 0.0), float(rule.get("minWeightSum") or 0.0), int(rule.get("minPixels") or 0),
                                  int(rule.get("minSumQ") or 0))
        check(self.device.lib.wdgs_densify_prune_encode_contribution_decision(self.handle, n, statsBuffer.ptr, C.byref(r)))
        self.numPoints = n
        b = self._buffers()
        return dict(actionBuffer=b["actionBuffer"], outCountBuffer=b["outCountBuffer"])

    def encodePrefixSum(self, encoder) -> HipBuffer:
        check(self.device.lib.wdgs_densify_prune_encode_prefix_sum(self.handle, self.numPoints))
        return self._buffers()["outOffsetBuffer"]

    def encodeCapToMax(self, encoder, outOffsetBuffer: Optional[HipBuffer], maxOutPoints: int) -> None:
        check(self.device.lib.wdgs_densify_prune_encode_cap_to_max(self.handle, self.numPoints, max(0, int(maxOutPoints))))

    def encodeTotalOut(self, encoder, outOffsetBuffer: Optional[HipBuffer] = None) -> HipBuffer:
        check(self.device.lib.wdgs_densify_prune_encode_total_out(self.handle, self.numPoints))
        return self._buffers()["outTotalBuffer"]

    def getOutTotalBuffer(self) -> HipBuffer:
        return self._buffers()["outTotalBuffer"]

    def getActionBuffer(self) -> HipBuffer:
        return self._buffers()["actionBuffer"]

    def getOutCountBuffer(self) -> HipBuffer:
        return self._buffers()["outCountBuffer"]

    def readTotal(self) -> int:
        t = C.c_uint32(0)
        check(self.device.lib.wdgs_densify_prune_read_total(self.handle, C.byref(t)))
        return int(t.value)

    def encodeScatter(self, encoder, inputs: dict, outputs: dict) -> None:
        pc: PointCloud = inputs["pointCloud"]
        out_pc: PointCloud = outputs["outPointCloud"]
        out_n = int(inputs["outNumPoints"])
        if out_pc.num_points != out_n:
            raise _lib.WdgsError(_lib.WDGS_E_INVALID, f"encodeScatter: outPointCloud.num_points ({out_pc.num_points}) != outNumPoints ({out_n})")
        in_st, out_st = inputs.get("optimizerState"), outputs.get("outOptimizerState")
        a = C.byref(_state_struct(in_st)) if in_st else None
        b = C.byref(_state_struct(out_st)) if out_st else None
        check(self.device.lib.wdgs_densify_prune_encode_scatter(self.handle, pc.num_points, pc.gaussian_3d_buffer.ptr, pc.sh_buffer.ptr, a, out_n,
                                                                1 if inputs.get("resetNewOptimizerState", True) else 0, out_pc.gaussian_3d_buffer.ptr,
                                                                out_pc.sh_buffer.ptr, b))

    def applyActions(self, *_a, **_k):
        raise NotImplementedError("DensifyPrunePass.applyActions is unimplemented in the reference (densify-prune.ts:680-686)")

    def destroy(self) -> None:
        if self.handle:
            self.device.lib.wdgs_densify_prune_destroy(self.handle)
            self.handle = None
