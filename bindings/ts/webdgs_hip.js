'use strict';
/*
 * webdgs_hip.js (+ webdgs_hip.d.ts) -- drop-in module for the reference's operator layer (src/renderers/tiled-forward-pass.ts,
 * tiled-rasterizer.ts, tiled-backward-pass.ts, optimizer.ts, densify-prune.ts, src/sort/sort_dynamic.ts, src/prefix/prefix.ts,
 * src/utils/allocate-pointcloud.ts) backed by the N-API addon over libwebdgs_hip.so.
 *
 * Same class names, constructor shapes and method names as the reference; GPUDevice / GPUBuffer / GPUTextureView /
 * GPUCommandEncoder / GPUCommandBuffer become HipDevice / HipBuffer / HipEncoder / HipCommandBuffer.  A src/trainer.ts that imports
 * these instead of the WebGPU classes needs no other change than the import lines (INTEGRATION.md); bindings/ts/trainer.js is that
 * trainer, already rewritten.  Shipped as JavaScript with hand-written typings, the way an npm package reaches a TypeScript host:
 * there is no tsc in this repository's image, but plain CommonJS RUNS here (node 12: no `?.`, no `??`), so the module is executed
 * end to end on the GPU by tests/test_gpu_napi.py instead of merely being written.
 */
const path = require('path');
const addon = require(path.join(__dirname, '..', 'napi', 'webdgs_napi.node'));

const dflt = (v, d) => (v === undefined || v === null ? d : v);

class HipBuffer {                        // GPUBuffer
  constructor(device, ptr, size, handle) {
    this.device = device; this.ptr = ptr; this.size = size; this.handle = handle; this.destroyed = false;
    // called before the buffer's CONTENT is handed to the host (HipDevice.readBuffer / readBufferAsync) or copied by copyBufferToBuffer: a producer
    // that keeps part of it elsewhere brings it up to date first (the optimizer's deferred SH writes and compact training copy)
    this.beforeRead = null;
  }
  /** mapAsync + getMappedRange in one synchronous call: the buffer's bytes as an ArrayBuffer. */
  read(byteLength) { return this.device.readBuffer(this, byteLength); }
  destroy() {
    if (this.destroyed) return;
    this.destroyed = true;
    if (this.handle !== undefined) addon.bufferDestroy(this.handle);
  }
}

/** GPUCommandBuffer backed by an instantiated HIP graph; unlike WebGPU's it may be submitted again (all sizes are read on the device). */
class HipCommandBuffer {
  constructor(device, handle) { this.device = device; this.handle = handle; }
  destroy() { if (this.handle !== null) { addon.commandBufferDestroy(this.handle); this.handle = null; } }
}

/** GPUCommandEncoder.  Default (eager): encodes go to the HIP stream as they are made; `record: true` captures them into a graph. */
class HipEncoder {
  constructor(device, label, record) {
    this.device = device; this.label = label || ''; this.record = !!record; this.open = false;
    if (this.record) { addon.encoderBegin(device.handle); this.open = true; }
  }
  clearBuffer(buffer) { addon.bufferClear(this.device.handle, buffer.ptr, buffer.size); }
  /** encoder.copyBufferToBuffer (trainer.ts:445): device to device, stream-ordered, recordable. */
  copyBufferToBuffer(src, srcOffset, dst, dstOffset, size) {
    if (srcOffset + size > src.size || dstOffset + size > dst.size) throw new RangeError('copyBufferToBuffer: range exceeds a buffer');
    if (src.beforeRead) src.beforeRead();
    addon.copyBufferToBuffer(this.device.handle, dst.ptr + BigInt(dstOffset), src.ptr + BigInt(srcOffset), size);
  }
  finish() {
    if (!this.record) return new HipCommandBuffer(this.device, null);
    this.open = false;
    return new HipCommandBuffer(this.device, addon.encoderFinish(this.device.handle));
  }
  /** Drops an unfinished recording (an encode threw): the device goes back to eager mode.  No-op otherwise. */
  abort() { if (this.open) { this.open = false; addon.encoderAbort(this.device.handle); } }
}

// capacity reports and the growth rule of tile-entry lists: plain JavaScript of its own (loadable without the addon), re-exported below
const { CapacityReports, grownTileEntries } = require('./capacity_reports.js');

class HipDevice {                        // GPUDevice + GPUQueue
  constructor(ordinal) {
    this.handle = addon.deviceCreate(ordinal || 0);
    this.capacityReports = new CapacityReports();
    const self = this;
    this.queue = {
      submit(cmds) { for (const c of cmds) if (c.handle !== null) addon.queueSubmit(self.handle, c.handle); },
      onSubmittedWorkDone() { return addon.queueOnSubmittedWorkDone(self.handle); },   // Promise, resolved from the HIP runtime thread
      mark() { return addon.queueMark(self.handle); },                                  // a ticket for the work submitted so far ...
      wait(ticket) { addon.queueWait(self.handle, ticket); },                           // ... awaited later (blocking; raises deferred capacity errors)
      writeBuffer(buffer, offset, data) { addon.copyToDevice(self.handle, buffer.ptr + BigInt(offset), data); },
    };
  }
  createBuffer(desc) {
    const b = addon.bufferCreate(this.handle, desc.size);
    return new HipBuffer(this, b.ptr, desc.size, b.handle);
  }
  createCommandEncoder(desc) { return new HipEncoder(this, desc && desc.label, desc && desc.record); }
  view(ptr, size) { return new HipBuffer(this, ptr, size, undefined); }
  readBuffer(buffer, byteLength) {
    if (buffer.beforeRead) buffer.beforeRead();
    return addon.copyToHost(this.handle, buffer.ptr, byteLength === undefined ? buffer.size : byteLength);
  }
  /** Pinned host memory (wdgs_host_alloc) as an ArrayBuffer: the destination of readBufferAsync. */
  createPinnedArrayBuffer(byteLength) { return addon.hostAlloc(byteLength); }
  /** mapAsync(READ) counterpart (trainer.ts:455-458): queues the copy and resolves once the stream reaches it. */
  readBufferAsync(buffer, offset, pinned, byteLength) {
    if (buffer.handle === undefined) throw new Error('readBufferAsync needs a buffer created by createBuffer');
    if (buffer.beforeRead) buffer.beforeRead();
    addon.bufferReadAsync(this.handle, buffer.handle, offset, pinned, byteLength);
    return addon.queueOnSubmittedWorkDone(this.handle).then(() => pinned);
  }
  /** Blocking variant of onSubmittedWorkDone; also raises deferred capacity errors (code WDGS_E_CAPACITY). */
  synchronize() { addon.deviceSynchronize(this.handle); }
  /** device.limits as far as memory goes (trainer.ts:147): { free, total, cached } in bytes; cached = what the library's allocation cache holds. */
  memoryInfo() { return addon.deviceMemoryInfo(this.handle); }
  selectLane(lane) { addon.deviceSelectLane(this.handle, lane); }            // include/webdgs.h "Lanes"
  laneOrder(waiter, signal) { addon.deviceLaneOrder(this.handle, waiter, signal); }
  laneMark(lane, mark) { addon.deviceLaneMark(this.handle, lane, mark); }          // remembers the current end of `lane` in mark `mark` ...
  laneWaitMark(lane, mark) { addon.deviceLaneWaitMark(this.handle, lane, mark); }  // ... for lanes that wait for it later
  /** Per-kernel hipEvent timing (wdgs_device_set_profiling): kernelTimes() -> { name: { launches, totalMs } } after a synchronize. */
  setProfiling(enabled) { addon.deviceKernelTimes(this.handle, enabled ? 1 : 0); }
  kernelTimes(reset) { const t = addon.deviceKernelTimes(this.handle, 3); if (reset) addon.deviceKernelTimes(this.handle, 2); return t; }
  destroy() { if (this.handle !== null) { addon.encoderAbort(this.handle); addon.deviceDestroy(this.handle); this.handle = null; } }
}

/** allocatePointCloudLike (src/utils/allocate-pointcloud.ts:8-44): zeroed buffers of the template's layout for `numPoints`. */
function allocatePointCloudLike(device, template, options) {
  const n = Math.max(1, Math.floor(options.numPoints));
  const tp = Math.max(1, template.num_points);
  const bpg = Math.max(1, Math.floor(template.gaussian_3d_buffer.size / tp));
  const bps = Math.max(1, Math.floor(template.sh_buffer.size / tp));
  return { type: template.type || 'normal', num_points: n, sh_deg: template.sh_deg || 0,
    gaussian_3d_buffer: device.createBuffer({ size: n * bpg }), sh_buffer: device.createBuffer({ size: n * bps }) };
}

class PrefixScanner {                    // src/prefix/prefix.ts:26-43
  constructor(maxElements, device) {
    const s = addon.prefixScanner(0, device.handle, maxElements);
    this.device = device; this.handle = s.handle; this.max_elements = maxElements;
    this.input_buffer = device.view(s.inputBuffer, 4 * maxElements);
    this.output_buffer = device.view(s.outputBuffer, 4 * maxElements);
  }
  set_count(count) { addon.prefixScanner(1, this.handle, count); return { num_workgroups: Math.ceil(count / 4096) }; }
  scan(_encoder) { addon.prefixScanner(2, this.handle, 0); }
  destroy() { if (this.handle !== null) { addon.prefixScanner(3, this.handle, 0); this.handle = null; } }
}
/** get_prefix_scanner(maxElements, device): PrefixScanner (prefix.ts:140) */
function get_prefix_scanner(maxElements, device) { return new PrefixScanner(maxElements, device); }

class DynamicSortStuff {                 // src/sort/sort_dynamic.ts:9-24 -- the element count is read on the device from statsBuffer[0]
  constructor(maxCapacity, device, statsBuffer) {
    const s = addon.dynamicSorter(0, device.handle, maxCapacity, statsBuffer.ptr);
    this.device = device; this.handle = s.handle; this.capacity = s.capacity; this.final_out_index = 0;
    this.ping_pong = [
      { sort_depths_buffer: device.view(s.keys0, 4 * s.capacity), sort_indices_buffer: device.view(s.values0, 4 * s.capacity) },
      { sort_depths_buffer: device.view(s.keys1, 4 * s.capacity), sort_indices_buffer: device.view(s.values1, 4 * s.capacity) }];
  }
  sort(_encoder, keyBits) { this.final_out_index = addon.dynamicSorter(1, this.handle, dflt(keyBits, 32), 0); }
  destroy() { if (this.handle !== null) { addon.dynamicSorter(2, this.handle, 0, 0); this.handle = null; } }
}
/** get_dynamic_sorter(maxCapacity, device, statsBuffer): DynamicSortStuff (sort_dynamic.ts:252) */
function get_dynamic_sorter(maxCapacity, device, statsBuffer) { return new DynamicSortStuff(maxCapacity, device, statsBuffer); }

class TiledForwardPass {                 // tiled-forward-pass.ts:62
  constructor(device, pointCloud, cameraBuffer, config) {
    this.device = device; this.pointCloud = pointCloud; this.cameraBuffer = cameraBuffer; this.destroyed = false;
    this.handle = addon.tiledForwardCreate(device.handle, {
      numPoints: pointCloud.num_points, shDeg: pointCloud.sh_deg || 0, viewportWidth: config.viewportWidth, viewportHeight: config.viewportHeight,
      gaussianScale: dflt(config.gaussianScale, 1.0), pointSizePx: dflt(config.pointSizePx, 3.0), maxSplatRadiusPx: dflt(config.maxSplatRadiusPx, 128.0),
      renderMode: dflt(config.renderMode, 'gaussian') === 'gaussian' ? 1 : 0, maxTileEntries: config.maxTileEntries || 0, compatCaps: config.compatCaps ? 1 : 0,
    });
  }
  get nativeHandle() { return this.handle; }
  /** K1 takes the SH-DC halves from the optimizer's compact array (Optimizer.setDeferredSH) instead of the cloud's rows; null restores the rows. */
  setDcSource(dcWords) { this.dcSource = dcWords || null; addon.tiledForwardSetDcSource(this.handle, dcWords ? dcWords.ptr : null); }
  /** A cloud that is being trained with deferred SH writes carries the optimizer's compact array (pointCloud.dcWords, Optimizer.setDeferredSH):
   *  every forward pass built on that cloud -- the trainer's, a Viewer's -- takes the SH-DC halves from it without the host knowing. */
  syncDcSource() { const want = this.pointCloud.dcWords || null; if (want !== (this.dcSource || null)) this.setDcSource(want); }
  encode(_encoder, options) {
    this.syncDcSource();
    addon.tiledForwardEncode(this.handle, this.pointCloud.gaussian_3d_buffer.ptr, this.pointCloud.sh_buffer.ptr, this.cameraBuffer.ptr, options && options.skipSort ? 1 : 0);
  }
  /** The rest of encode (scan, emit, sort) for a pass whose K1 ran through projectViews (view-batched step; no reference counterpart). */
  encodeProjected(_encoder) { addon.tiledForwardEncodeProjected(this.handle); }
  isProjected() { return addon.tiledForwardIsProjected(this.handle) !== 0; }
  setCameraBuffer(buffer) { this.cameraBuffer = buffer; }
  /** Adopts a point cloud of another size (wdgs_tiled_forward_resize) instead of destroy + construct; false if the SH degree differs. */
  setPointCloud(pointCloud) {
    if ((pointCloud.sh_deg || 0) !== (this.pointCloud.sh_deg || 0)) return false;
    addon.tiledForwardResize(this.handle, pointCloud.num_points); this.pointCloud = pointCloud; return true;
  }
  setRenderMode(mode) { addon.tiledForwardSet(this.handle, 0, mode === 'gaussian' ? 1 : 0); }
  setPointSize(value) { addon.tiledForwardSet(this.handle, 1, value); }
  setGaussianScale(value) { addon.tiledForwardSet(this.handle, 2, value); }
  setViewport(width, height) { addon.tiledForwardSetViewport(this.handle, width, height); }
  getResources() {
    const r = addon.tiledForwardGetResources(this.handle); const n = Math.max(1, this.pointCloud.num_points); const d = this.device;
    return { splatBuffer: d.view(r.splatBuffer, 24 * n), tileKeysBuffer: d.view(r.tileKeysBuffer, 4 * r.maxTileEntries), tileIndicesBuffer: d.view(r.tileIndicesBuffer, 4 * r.maxTileEntries),
      tileOffsetsBuffer: d.view(r.tileOffsetsBuffer, 4 * n), tileCountsBuffer: d.view(r.tileCountsBuffer, 4 * n), statsBuffer: d.view(r.statsBuffer, 16),
      numTilesX: r.numTilesX, numTilesY: r.numTilesY, totalTiles: r.totalTiles, maxTileEntries: r.maxTileEntries };
  }
  getSortedIndicesBuffer() { return this.getResources().tileIndicesBuffer; }
  getSortedKeysBuffer() { return this.getResources().tileKeysBuffer; }
  getTileOffsetsBuffer() { return this.getResources().tileOffsetsBuffer; }
  getStatsBuffer() { return this.getResources().statsBuffer; }
  /** Synchronises; throws (code WDGS_E_CAPACITY) if an encode since the last check overflowed maxTileEntries. */
  check() { return addon.tiledForwardCheck(this.handle); }
  /** Long tile lists (include/webdgs.h: wdgs_tiled_forward_set_long_lists): tiles with more than `threshold` entries get per-pixel lists (0: off). */
  setLongLists(threshold, maxItems, maxRows) { addon.tiledForwardSetLongLists(this.handle, threshold, maxItems || 0, maxRows || 0); }
  /** The last frame's long-list work: what it wanted and what the pass has room for (synchronises). */
  longListStats() { return addon.tiledForwardLongListStats(this.handle); }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.tiledForwardDestroy(this.handle); this.handle = null; }   // (a call after destroy meets the library's null check, not freed memory)
}

const DEPTH_KINDS = { expected: 1, median: 2, weight_sum: 4 };   // WDGS_DEPTH_*
const NO_NORMAL = 0x80008000;   // the packed word of a Gaussian without a normal (include/webdgs.h)
const CONTRIBUTION_RECORD_BYTES = 16;   // { u64 sum_q; u32 max_bits; u32 pixels } per Gaussian (include/webdgs.h)
function depthMask(kinds) {
  if (typeof kinds === 'number') return kinds;
  let mask = 0;
  for (const k of (typeof kinds === 'string' ? [kinds] : kinds)) {
    if (!(k in DEPTH_KINDS)) throw new Error(`unknown depth kind '${k}': one of ${Object.keys(DEPTH_KINDS).join(', ')}`);
    mask |= DEPTH_KINDS[k];
  }
  return mask;
}

class TiledRasterizer {                  // tiled-rasterizer.ts:34
  constructor(config) {
    this.device = config.device; this.forwardPass = config.forwardPass; this.destroyed = false; this.w = 0; this.h = 0;
    this.handle = addon.tiledRasterizerCreate(config.device.handle, config.forwardPass.nativeHandle);
  }
  encode(_encoder, width, height) { addon.tiledRasterizerEncode(this.handle, width, height); this.w = width; this.h = height; }
  getOutputTextureView() { return this.device.view(addon.tiledRasterizerGet(this.handle, 0), 4 * this.w * this.h); }      // throws before the first encode
  getAlphaTextureView() { return this.device.view(addon.tiledRasterizerGet(this.handle, 1), 4 * this.w * this.h); }
  getNContribTextureView() { return this.device.view(addon.tiledRasterizerGet(this.handle, 2), 4 * this.w * this.h); }
  getTileOffsetsBuffer() { return this.device.view(addon.tiledRasterizerGet(this.handle, 3), 4 * (Math.ceil(this.w / 16) * Math.ceil(this.h / 16) + 1)); }
  /** Depth images of the frame the last encode rasterized (include/webdgs.h, DESIGN.md section 10; no reference counterpart): `kinds` is an array of
   *  DEPTH_KINDS names ('expected' | 'median' | 'weight_sum'), one name, or the bit mask.  The first use of a kind allocates its image and cannot be recorded. */
  encodeDepth(_encoder, kinds) { addon.tiledRasterizerEncodeDepth(this.handle, depthMask(kinds === undefined ? ['expected'] : kinds)); }
  /** f32[W*H] of one kind the last encodeDepth wrote; throws (WDGS_E_STATE) otherwise. */
  getDepthTextureView(kind) { return this.device.view(addon.tiledRasterizerGetDepth(this.handle, depthMask([kind === undefined ? 'expected' : kind])), 4 * this.w * this.h); }
  /** The normal map of the frame the last encode rasterized (include/webdgs.h, DESIGN.md section 12; no reference counterpart): one packed view-space
   *  normal per Gaussian of the forward pass's cloud under its camera, composited with the colour image's weights.  The first use, and the first after
   *  the point count or the size changed, allocates and cannot be recorded. */
  encodeNormal(_encoder) { addon.tiledRasterizerEncodeNormal(this.handle, this.forwardPass.pointCloud.gaussian_3d_buffer.ptr, this.forwardPass.cameraBuffer.ptr); }
  /** rgba32f[W*H] { N.x, N.y, N.z, A } of the last encodeNormal (N un-normalised: |N| <= A); throws (WDGS_E_STATE) before it. */
  getNormalTextureView() { return this.device.view(addon.tiledRasterizerGetNormal(this.handle, 0), 16 * this.w * this.h); }
  /** u32[numPoints]: the packed per-Gaussian normals of the last encodeNormal (0x80008000: no normal); throws (WDGS_E_STATE) before it. */
  getGaussianNormals() { return this.device.view(addon.tiledRasterizerGetNormal(this.handle, 1), 4 * Math.max(1, this.forwardPass.pointCloud.num_points)); }
  /** Adds the per-Gaussian contribution of the frame the last encode rasterized into `statsBuffer` (createContributionBuffer; include/webdgs.h,
   *  DESIGN.md section 11; no reference counterpart).  Allocates nothing, so it records. */
  encodeContribution(_encoder, statsBuffer) {
    const n = this.forwardPass.pointCloud.num_points;
    if (statsBuffer.size < CONTRIBUTION_RECORD_BYTES * n) throw new Error(`encodeContribution: the statistics buffer holds ${statsBuffer.size} bytes, ${n} Gaussians need ${CONTRIBUTION_RECORD_BYTES * n}`);
    addon.tiledRasterizerEncodeContribution(this.handle, statsBuffer.ptr);
  }
  /** blitToTexture(encoder, targetView, clearColor?) (tiled-rasterizer.ts:333-357): `target` is an rgba8 image buffer; it may carry its own
   *  `width` / `height` (a canvas of another size: the blit is a bilinear resample), otherwise it has the rasterizer's size.  The blit covers
   *  the whole target, so the reference's clear colour never shows and is accepted only for signature compatibility. */
  blitToTexture(_encoder, target, _clearColor) { addon.tiledRasterizerBlit(this.handle, target.ptr, dflt(target.width, this.w), dflt(target.height, this.h)); }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.tiledRasterizerDestroy(this.handle); this.handle = null; }
}

const resourcePtrs = (r) => ({ splatBuffer: r.splatBuffer.ptr, tileOffsetsBuffer: r.tileOffsetsBuffer.ptr, tileIndicesBuffer: r.tileIndicesBuffer.ptr,
  cameraBuffer: r.cameraBuffer ? r.cameraBuffer.ptr : null, alphaTexture: r.alphaTexture ? r.alphaTexture.ptr : null, nContribTexture: r.nContribTexture.ptr });

class TiledBackwardPass {                // tiled-backward-pass.ts:71
  constructor(device, pointCloud, config) {
    const t = config.trainingConfig;
    this.device = device; this.pointCloud = pointCloud; this.destroyed = false; this.w = config.viewportWidth; this.h = config.viewportHeight;
    this.handle = addon.tiledBackwardCreate(device.handle, { numPoints: pointCloud.num_points, shDeg: pointCloud.sh_deg || 0, viewportWidth: config.viewportWidth,
      viewportHeight: config.viewportHeight, lambda_l1: t.lambda_l1, lambda_l2: t.lambda_l2, lambda_dssim: t.lambda_dssim, c1: dflt(t.c1, 0.0001), c2: dflt(t.c2, 0.0009),
      dssim_mode: dflt(t.dssim_mode, 'reference'), maxSplatRadiusPx: dflt(config.maxSplatRadiusPx, 128.0) });
    this.trainingConfig = { lambda_l1: t.lambda_l1, lambda_l2: t.lambda_l2, lambda_dssim: t.lambda_dssim, c1: dflt(t.c1, 0.0001), c2: dflt(t.c2, 0.0009),
      dssim_mode: dflt(t.dssim_mode, 'reference') };
  }
  encode(_encoder, predictedTexture, targetTexture, r, _options) {   // (TiledBackwardPassOptions is an empty interface in the reference)
    addon.tiledBackwardEncode(this.handle, predictedTexture.ptr, targetTexture.ptr, resourcePtrs(r), this.pointCloud.gaussian_3d_buffer.ptr);
  }
  /** First half of encode (K15 loss gradient, clear, K16 backward raster): wdgs_tiled_backward_encode_raster. */
  encodeRaster(_encoder, predictedTexture, targetTexture, r) { addon.tiledBackwardEncodeRaster(this.handle, predictedTexture.ptr, targetTexture.ptr, resourcePtrs(r)); }
  /** Second half (K17).  `accumulate` (a batched step) = { sums, visible, tileCounts, guard, stats, first }: K17 also adds the view's gradient to the
   *  step's fp32 block and folds the forward pass's overflow word (stats + 8 bytes) into the guard word. */
  encodeGeometry(_encoder, cameraBuffer, accumulate) {
    const a = accumulate ? { sums: accumulate.sums.ptr, visible: accumulate.visible.ptr, tileCounts: accumulate.tileCounts.ptr, guard: accumulate.guard.ptr,
      overflowWord: accumulate.stats.ptr + 8n, first: accumulate.first ? 1 : 0 } : null;
    addon.tiledBackwardEncodeGeometry(this.handle, cameraBuffer.ptr, this.pointCloud.gaussian_3d_buffer.ptr, a);
  }
  /** Whether Optimizer.stepWithGeometry also writes K17's packed gradient to getGradientsBuffer() (default: yes, as the reference's K17 does). */
  setGradientOutput(enabled) { this.gradientOutput = !!enabled; addon.tiledBackwardSetGradientOutput(this.handle, enabled ? 1 : 0); }
  /** computeMetricCounts of this pass adds into `counts` (another pass's getMetricCountsBuffer()) instead of its own array; null restores its own.
   *  Several passes can then take the metric views of one densify event on different lanes (integer atomics: any order gives the same bits). */
  setMetricCountsTarget(counts) { this.metricTarget = counts || null; addon.tiledBackwardSetMetricCountsTarget(this.handle, counts ? counts.ptr : null); }
  /** setTrainingConfig(next) (tiled-backward-pass.ts:812-830): loss weights and dssim_mode of the next encode. */
  setTrainingConfig(next) {
    const cfg = Object.assign({ lambda_l1: 0.8, lambda_l2: 0.0, lambda_dssim: 0.2, c1: 0.0001, c2: 0.0009, dssim_mode: 'reference' }, this.trainingConfig || {}, next || {});
    addon.tiledBackwardMetric(this.handle, 5, cfg, 0, 0);   // (throws for an unknown dssim_mode before it changes anything)
    this.trainingConfig = cfg;
  }
  /** See TiledForwardPass.setPointCloud (wdgs_tiled_backward_resize). */
  setPointCloud(pointCloud) {
    if ((pointCloud.sh_deg || 0) !== (this.pointCloud.sh_deg || 0)) return false;
    addon.tiledBackwardResize(this.handle, pointCloud.num_points); this.pointCloud = pointCloud; return true;
  }
  computeLossOnly(_encoder, predicted, target) { addon.tiledBackwardMetric(this.handle, 0, predicted.ptr, target.ptr, 0); }
  computeMetricMap(_encoder, predicted, target, options) { addon.tiledBackwardMetric(this.handle, 1, predicted.ptr, target.ptr, dflt(options && options.threshold, 0.5)); }
  computeMetricCounts(_encoder, r, options) {
    addon.tiledBackwardMetric(this.handle, 2, resourcePtrs(r), (options && options.numInstances) || Math.floor(r.tileIndicesBuffer.size / 4), options && options.clear === false ? 0 : 1);
  }
  normalizeMetricCounts(_encoder, options) { addon.tiledBackwardMetric(this.handle, 3, Math.max(1, Math.floor(options.divisor)), 0, 0); }
  setViewport(width, height) { addon.tiledBackwardMetric(this.handle, 4, width, height, 0); this.w = width; this.h = height; }
  getGradientsBuffer() { return this.device.view(addon.tiledBackwardGet(this.handle, 0), 32 * Math.max(1, this.pointCloud.num_points)); }
  getMetricCountsBuffer() { return this.device.view(addon.tiledBackwardGet(this.handle, 1), 4 * Math.max(1, this.pointCloud.num_points)); }
  getLossTextureView() { return this.device.view(addon.tiledBackwardGet(this.handle, 2), 16 * this.w * this.h); }
  getMetricMapTextureView() { return this.device.view(addon.tiledBackwardGet(this.handle, 3), 4 * this.w * this.h); }
  getMetricMapTexture() { return this.getMetricMapTextureView(); }   // (texture and view are the same r32uint image buffer here)
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.tiledBackwardDestroy(this.handle); this.handle = null; }
}

const DEFAULT_ADAM_HYPERPARAMETERS = { lr_pos: 0.00016, lr_color: 0.0025, lr_opacity: 0.05, lr_scale: 0.005, lr_rot: 0.001, beta1: 0.9, beta2: 0.999, epsilon: 1e-8 };  // adam-config.ts:12-21
const STATE_KEYS = ['optPosBuffer', 'optRotBuffer', 'optScaleBuffer', 'optOpacityBuffer', 'paramSH', 'stateSH'];
const statePtrs = (s) => { const o = {}; for (const k of STATE_KEYS) o[k] = s[k].ptr; return o; };

/** allocateOptimizerStateBuffers (optimizer.ts:27-38). */
function allocateOptimizerStateBuffers(device, numPoints) {
  const sizes = addon.optimizerStateSizes(Math.max(1, numPoints));
  const o = {};
  STATE_KEYS.forEach((k, i) => { o[k] = device.createBuffer({ size: sizes[i] }); });
  return o;
}

class Optimizer {                        // optimizer.ts:40
  /** `initialState` = { iteration, buffers } is ADOPTED as-is (OptimizerInitialState, optimizer.ts:22-25, 81-88). */
  constructor(device, pointCloud, params, initialState) {
    this.device = device; this.pointCloud = pointCloud; this.destroyed = false;
    this.buffers = initialState && initialState.buffers ? initialState.buffers : null;
    this.handle = this.buffers
      ? addon.optimizerCreateWithState(device.handle, pointCloud.num_points, pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr, statePtrs(this.buffers), 0,
                                       initialState.iteration || 0)
      : addon.optimizerCreate(device.handle, pointCloud.num_points, pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr);
    if (params) addon.optimizerHyperparameters(this.handle, params);
  }
  getIteration() { return addon.optimizerGetIteration(this.handle); }
  getHyperparameters() { return addon.optimizerHyperparameters(this.handle, null); }
  setHyperparameters(next) { addon.optimizerHyperparameters(this.handle, next); }
  /** Brings the SH-DC rows of paramSH / stateSH up to date before handing the arrays out (see include/webdgs.h). */
  getStateBuffers() {
    const s = addon.optimizerState(this.handle, 0);
    let o = this.buffers;
    if (!o) {
      const sizes = addon.optimizerStateSizes(Math.max(1, this.pointCloud.num_points));
      o = {};
      STATE_KEYS.forEach((k, i) => { o[k] = this.device.view(s[k], sizes[i]); });
    }
    // position, log-scale and SH-DC {param, m, v} are trained in a compact copy: a handle kept across steps is brought up to date whenever its
    // content is read through the host (the reference's GPUBuffers are live)
    const self = this;
    for (const k of STATE_KEYS) if (!o[k].beforeRead) o[k].beforeRead = () => { if (!self.destroyed) addon.optimizerState(self.handle, 0); };
    return o;
  }
  step(_encoder, coefficients, gradientsBuffer, tileCountsBuffer) {
    addon.optimizerStep(this.handle, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, gradientsBuffer.ptr, tileCountsBuffer.ptr);
  }
  /** Deferred SH writes (include/webdgs.h wdgs_optimizer_set_deferred_sh): on, step() writes the trained SH-DC halves to a compact array
   *  (returned: give it to every forward pass that renders the cloud, TiledForwardPass.setDcSource) instead of 6 bytes into every 96-byte
   *  row; flushSH(pointCloud) brings the rows up to date -- call it before anything reads pointCloud.sh_buffer (a host read, an export, a
   *  viewer's own forward pass, DensifyPrunePass.encodeScatter).  Off: flushes and restores the reference's write pattern. */
  setDeferredSH(pointCloud, enabled) {
    const on = enabled !== false;
    const p = addon.optimizerDeferredSH(this.handle, pointCloud.sh_buffer.ptr, on ? 1 : 0);
    this.deferredCloud = on ? pointCloud : null;
    const words = on && p !== null ? this.device.view(p, 8 * Math.max(1, this.pointCloud.num_points)) : null;
    const self = this;
    pointCloud.sh_buffer.beforeRead = on ? () => self.flushSH(pointCloud) : null;   // host reads of the rows see the trained values
    pointCloud.dcWords = words;                                                   // forward passes built on the cloud pick the halves up (syncDcSource)
    return words;
  }
  flushSH(pointCloud) { if (!this.destroyed) addon.optimizerFlushSH(this.handle, pointCloud.sh_buffer.ptr); }
  /** step() fused with K17 (wdgs_optimizer_step_with_geometry): call after backwardPass.encodeRaster for the view. */
  stepWithGeometry(_encoder, coefficients, backwardPass, cameraBuffer, tileCountsBuffer) {
    addon.optimizerStepWithGeometry(this.handle, backwardPass.handle, cameraBuffer.ptr, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, tileCountsBuffer.ptr);
  }
  /** Adam + re-pack on Gaussians [first, first + count) -- the slice a data-parallel rank owns; rowsOut also receives the re-packed 32-byte rows. */
  stepF32Range(_encoder, coefficients, gradF32, visibleCounts, first, count, rowsOut) {
    addon.optimizerStepF32Range(this.handle, coefficients.gaussian_3d_buffer.ptr, coefficients.sh_buffer.ptr, gradF32.ptr, visibleCounts.ptr, first, count, rowsOut ? rowsOut.ptr : null);
  }
  /** Writes the rows the other ranks published into this replica (with deferred SH writes the gathered halves go to the compact array). */
  applyRepackedRows(rows, skipFirst, skipCount, guard, pointCloud) {
    addon.optimizerApplyRepackedRows(this.handle, rows.ptr, skipFirst, skipCount, guard ? guard.ptr : null, pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr);
  }
  /** The state arrays were rewritten from outside (slices gathered from other ranks, a restored snapshot): refresh the internal copies. */
  stateChanged() { addon.optimizerStateChanged(this.handle); }
  /** While the u32 at `flagBuffer + offset` is non-zero at execution time, step() leaves every buffer untouched (tile-entry overflow). */
  setGuard(flagBuffer, offset) { addon.optimizerSetGuard(this.handle, flagBuffer ? flagBuffer.ptr + BigInt(offset || 0) : null); }
  /** Host-side iteration counter: call when a recorded command buffer containing step() is re-submitted. */
  advanceIteration(count) { addon.optimizerAdvanceIteration(this.handle, dflt(count, 1)); }
  /** Also destroys adopted state buffers, as the reference's Optimizer.destroy() does (optimizer.ts:352-362). */
  destroy() {
    if (this.destroyed) return;
    if (this.deferredCloud && !this.deferredCloud.sh_buffer.destroyed) this.setDeferredSH(this.deferredCloud, false);  // the cloud outlives its optimizer: leave its rows current
    this.destroyed = true;
    addon.optimizerDestroy(this.handle);
    this.handle = null;
    if (this.buffers) for (const k of STATE_KEYS) this.buffers[k].destroy();
  }
}

class DensifyPrunePass {                 // densify-prune.ts:75
  constructor(device, config) {
    this.device = device; this.numPoints = 0;
    this.config = Object.assign({ strategy: 'cpu_rebuild', numViews: 1, cloneThreshold: 0, pruneThreshold: 0, maxNewPointsPerStep: 0, maxBufferBytes: 128 * 1024 * 1024 }, config || {});
    this.handle = addon.densifyCreate(device.handle, this.config);
  }
  setConfig(next) { this.config = Object.assign({}, this.config, next); addon.densifySetConfig(this.handle, this.config); }
  getConfig() { return Object.assign({}, this.config); }
  wrap(p, n) {
    const d = this.device; const m = Math.max(1, n);
    return { actionBuffer: d.view(p.actionBuffer, 4 * m), outCountBuffer: d.view(p.outCountBuffer, 4 * m), outOffsetBuffer: d.view(p.outOffsetBuffer, 4 * m),
      outTotalBuffer: d.view(p.outTotalBuffer, 4), maxOutPoints: p.maxOutPoints };
  }
  encodePrepare(_encoder, inputs) {
    const n = inputs.pointCloud.num_points; this.numPoints = n;
    return this.wrap(addon.densifyEncodePrepare(this.handle, n, inputs.pointCloud.gaussian_3d_buffer.ptr, inputs.metricCountsBuffer ? inputs.metricCountsBuffer.ptr : null), n);
  }
  // ---- the stages encodePrepare is made of (densify-prune.ts:327-456), individually recordable as in the reference
  stage(stage, n, a, b) { return this.wrap(addon.densifyStage(this.handle, stage, n, dflt(a, 0), dflt(b, 0)), n); }
  ensureSize(numPoints) { this.numPoints = numPoints; this.stage(4, numPoints); }
  computeMaxOutPoints(pointCloud) { return this.stage(4, pointCloud.num_points).maxOutPoints; }
  encodeDecision(_encoder, inputs) {
    this.numPoints = inputs.pointCloud.num_points;
    const p = this.stage(0, this.numPoints, inputs.pointCloud.gaussian_3d_buffer.ptr, inputs.metricCountsBuffer ? inputs.metricCountsBuffer.ptr : null);
    return { actionBuffer: p.actionBuffer, outCountBuffer: p.outCountBuffer };
  }
  /** The decision of contribution-based pruning (DESIGN.md section 11; no reference counterpart): a Gaussian is kept iff its record in `statsBuffer`
   *  meets every non-zero field of `rule` ({ minMaxWeight, minWeightSum, minPixels, minSumQ: number | bigint }).  encodePrefixSum, encodeTotalOut,
   *  readTotal and encodeScatter then compact the cloud; what this stage keeps is copied bit for bit. */
  encodeContributionDecision(_encoder, numPoints, statsBuffer, rule) {
    for (const k of Object.keys(rule)) if (!['minMaxWeight', 'minWeightSum', 'minPixels', 'minSumQ'].includes(k)) throw new Error(`encodeContributionDecision: unknown rule field '${k}'`);
    if (statsBuffer.size < CONTRIBUTION_RECORD_BYTES * numPoints) throw new Error(`encodeContributionDecision: the statistics buffer holds ${statsBuffer.size} bytes, ${numPoints} Gaussians need ${CONTRIBUTION_RECORD_BYTES * numPoints}`);
    const p = this.wrap(addon.densifyContributionDecision(this.handle, numPoints, statsBuffer.ptr, rule.minMaxWeight || 0, rule.minWeightSum || 0, rule.minPixels || 0, rule.minSumQ || 0), numPoints);
    this.numPoints = numPoints;
    return { actionBuffer: p.actionBuffer, outCountBuffer: p.outCountBuffer };
  }
  encodePrefixSum(_encoder) { return this.stage(1, this.numPoints).outOffsetBuffer; }
  encodeCapToMax(_encoder, _outOffsetBuffer, maxOutPoints) { this.stage(2, this.numPoints, Math.max(0, Math.floor(maxOutPoints))); }
  encodeTotalOut(_encoder, _outOffsetBuffer) { return this.stage(3, this.numPoints).outTotalBuffer; }
  /** The one 4-byte read-back of the densify path (trainer.ts:440-458, mapAsync on outTotalBuffer). */
  readTotal() { return addon.densifyReadTotal(this.handle); }
  encodeScatter(_encoder, inputs, outputs) {
    if (outputs.outPointCloud.num_points !== inputs.outNumPoints) throw new Error('encodeScatter: outPointCloud.num_points must equal outNumPoints');  // densify-prune.ts:478-480
    addon.densifyEncodeScatter(this.handle, inputs.pointCloud.num_points, inputs.pointCloud.gaussian_3d_buffer.ptr, inputs.pointCloud.sh_buffer.ptr,
      inputs.optimizerState ? statePtrs(inputs.optimizerState) : null, inputs.outNumPoints, inputs.resetNewOptimizerState === false ? 0 : 1,
      outputs.outPointCloud.gaussian_3d_buffer.ptr, outputs.outPointCloud.sh_buffer.ptr, outputs.outOptimizerState ? statePtrs(outputs.outOptimizerState) : null);
  }
  getActionBuffer() { return this.numPoints ? this.stage(4, this.numPoints).actionBuffer : null; }        // densify-prune.ts getters: null before ensureSize
  getOutCountBuffer() { return this.numPoints ? this.stage(4, this.numPoints).outCountBuffer : null; }
  getOutTotalBuffer() { return this.stage(4, Math.max(1, this.numPoints)).outTotalBuffer; }
  applyActions(_encoder) { throw new Error('DensifyPrunePass.applyActions is unimplemented in the reference (densify-prune.ts:680-686)'); }
  destroy() { if (this.handle !== null) { addon.densifyDestroy(this.handle); this.handle = null; } }
}

/** Bilinear blit of an rgba8 image to another size (trainer.ts:303-328: the ground-truth down-sample of the metric views). */
function downsampleRGBA8(device, src, srcW, srcH, dst, dstW, dstH) { addon.downsampleRGBA8(device.handle, src.ptr, srcW, srcH, dst.ptr, dstW, dstH); }

/** K1 of ALL the views of a batched step in one launch (wdgs_tiled_forward_project_views); follow with forwardPasses[v].encodeProjected(encoder). */
function projectViews(forwardPasses, cameraBuffers, pointCloud) {
  for (const f of forwardPasses) f.syncDcSource();
  addon.tiledForwardProjectViews(forwardPasses.map((f) => f.handle), cameraBuffers.map((c) => c.ptr), pointCloud.gaussian_3d_buffer.ptr, pointCloud.sh_buffer.ptr);
}
/** K17 of ALL the views of a batched step in one launch (wdgs_tiled_backward_encode_geometry_views): the step's fp32 gradient block, visibility counts
 *  and guard word, bit for bit what encodeGeometry(camera, { first: v === 0, ... }) per view produces. */
function geometryViews(backwardPasses, cameraBuffers, forwardPasses, sums, visible, guard, pointCloud, writeGradients, continues) {
  const res = forwardPasses.map((f) => addon.tiledForwardGetResources(f.handle));
  addon.tiledBackwardGeometryViews(backwardPasses.map((b) => b.handle), cameraBuffers.map((c) => c.ptr), res.map((r) => r.tileCountsBuffer), res.map((r) => r.statsBuffer + 8n),
    pointCloud.gaussian_3d_buffer.ptr, sums.ptr, visible.ptr, guard.ptr, writeGradients ? 1 : 0, continues ? 1 : 0);
}
/** Exact sum of squared rgb8 differences of two rgba8 images (synchronises); PSNR = 10 log10(255^2 3P / SSE). */
function imageSSE(device, a, b, numPixels) {
  const out = device.createBuffer({ size: 8 });
  addon.imageSSE(device.handle, a.ptr, b.ptr, numPixels, out.ptr);
  const v = new BigUint64Array(device.readBuffer(out, 8))[0];
  out.destroy();
  return Number(v);
}
function imagePSNR(device, a, b, numPixels) {
  const sse = imageSSE(device, a, b, numPixels);
  return sse === 0 ? Infinity : 10 * Math.log10(255 * 255 * 3 * numPixels / sse);
}
/** PSNR in dB of an rgb8 sum of squared differences over numPixels pixels; Infinity for 0. */
function psnrFromSSE(sse, numPixels) { return Number(sse) === 0 ? Infinity : 10 * Math.log10(255 * 255 * 3 * numPixels / Number(sse)); }
/** Stream-ordered SSE: the u64 sum into the first 8 bytes of `out` (no host wait). */
function encodeImageSSE(device, a, b, numPixels, out) { addon.imageSSE(device.handle, a.ptr, b.ptr, numPixels, out.ptr); }
/** Stream-ordered SSIM (wdgs_image_ssim_rgb8): the f64 mean into the first 8 bytes of `out`, the per-pixel, per-channel map (W*H*3 f32) into `map`
 *  when given.  No host wait. */
function encodeImageSSIM(device, a, b, width, height, out, map) {
  addon.imageSSIM(device.handle, a.ptr, b.ptr, width, height, out.ptr, map ? map.ptr : null);
}
/** SSIM of two rgba8 images over their rgb channels (11x11 Gaussian window, sigma 1.5, zero padding: the 3DGS convention); 1 when identical.
 *  `map`: optional W*H*3 f32 buffer for the per-pixel, per-channel values.  Synchronises.  No reference counterpart. */
function imageSSIM(device, a, b, width, height, map) {
  const out = device.createBuffer({ size: 8 });
  encodeImageSSIM(device, a, b, width, height, out, map);
  const v = new Float64Array(device.readBuffer(out, 8))[0];
  out.destroy();
  return v;
}

/** A depth image (f32, getDepthTextureView) as rgba8 for presentation: inverse depth between `near` (white) and `far` (black), depth 0 black, alpha 255
 *  (wdgs_depth_to_rgba8).  Stream-ordered; no reference counterpart. */
function depthToRGBA8(device, depth, width, height, near, far, target) { addon.depthToRgba8(device.handle, depth.ptr, width, height, near, far, target.ptr); }

// ---------------------------------------------------------------- TSDF fusion and mesh extraction (include/webdgs.h, DESIGN.md section 13; no reference counterpart)
/** A device TSDF volume (wdgs_tsdf_volume): an axis-aligned grid of dims = [nx, ny, nz] voxels of voxelSize in world space, x fastest, voxel (i, j, k)
 *  centred at origin + (i + .5, j + .5, k + .5) voxelSize.  integrate fuses one depth image per call; extractTriangles / extractMesh take the zero level
 *  set as triangles by marching tetrahedra.  options: { truncation (default 4 voxels), maxWeight (64), colour (true) }. */
class TSDFVolume {
  constructor(device, origin, voxelSize, dims, options) {
    const o = options || {};
    this.device = device;
    this.origin = Float32Array.from(origin);
    this.voxelSize = Math.fround(voxelSize);
    this.dims = Array.from(dims, (d) => Math.floor(d));
    if (this.origin.length !== 3 || this.dims.length !== 3) throw new Error('TSDFVolume: origin and dims must have three entries');
    this.truncation = Math.fround(o.truncation === undefined || o.truncation === null ? 4.0 * voxelSize : o.truncation);
    this.maxWeight = o.maxWeight === undefined || o.maxWeight === null ? 64.0 : o.maxWeight;
    this.colour = o.colour === undefined || o.colour === null ? true : !!o.colour;
    this.numVoxels = this.dims[0] * this.dims[1] * this.dims[2];
    this.destroyed = false;
    this.handle = addon.tsdfVolumeCreate(device.handle, this.origin[0], this.origin[1], this.origin[2], this.voxelSize, this.dims[0], this.dims[1], this.dims[2],
      this.truncation, this.maxWeight, this.colour ? 1 : 0);
  }
  /** The volume that covers the box [lo, hi] with voxels of voxelSize: origin lo, dimensions rounded up (at least 2). */
  static fromBounds(device, lo, hi, voxelSize, options) {
    if (!(voxelSize > 0) || ![0, 1, 2].every((a) => Number.isFinite(lo[a]) && Number.isFinite(hi[a]) && hi[a] > lo[a])) {
      throw new Error('TSDFVolume.fromBounds: needs finite lo < hi and a positive voxel size');
    }
    return new TSDFVolume(device, lo, voxelSize, [0, 1, 2].map((a) => Math.max(2, Math.ceil((hi[a] - lo[a]) / voxelSize))), options);
  }
  /** f32[nz][ny][nx].  Handing it out counts as a write of the volume: extractTriangles counts anew after it. */
  getTSDFBuffer() { return this.device.view(addon.tsdfVolumeGet(this.handle, 0), 4 * this.numVoxels); }
  getWeightBuffer() { return this.device.view(addon.tsdfVolumeGet(this.handle, 1), 4 * this.numVoxels); }
  /** f32[3][nz][ny][nx]: the r, g and b planes; throws (WDGS_E_STATE) for a volume without colour. */
  getColourBuffer() { return this.device.view(addon.tsdfVolumeGet(this.handle, 2), 12 * this.numVoxels); }
  /** tsdf = 1, weight = 0, colour = 0.  Stream-ordered. */
  reset() { addon.tsdfVolumeReset(this.handle); }
  /** Fuses one view: depth f32[H*W], camera the 68-float block on the device; options { weightSum, colour (rgba8), minWeightSum (0.5) }.  One pass over
   *  the volume, no atomics; allocates nothing, so it records; an eager call waits once (it checks the block's size). */
  integrate(depth, camera, width, height, options) {
    const o = options || {}, n = width * height;
    if (depth.size < 4 * n || (o.weightSum && o.weightSum.size < 4 * n) || (o.colour && o.colour.size < 4 * n) || camera.size < 272) {
      throw new Error(`TSDFVolume.integrate: buffers too small for ${width}x${height}`);
    }
    addon.tsdfVolumeIntegrate(this.handle, depth.ptr, o.weightSum ? o.weightSum.ptr : null, o.colour ? o.colour.ptr : null, width, height, camera.ptr,
      o.minWeightSum === undefined || o.minWeightSum === null ? 0.5 : o.minWeightSum);
  }
  /** Counts the mesh's triangles over the cells whose eight corners have weight >= minWeight (count, scan; waits). */
  countTriangles(minWeight) { return addon.tsdfVolumeCountTriangles(this.handle, minWeight === undefined || minWeight === null ? 1.0 : minWeight); }
  /** The raw device output: { positions: Float32Array[F*9], keys: BigUint64Array[F*3], colours: Uint8Array[F*12] | null, count: F }, triangles in cell,
   *  tetrahedron and case order, wound counter-clockwise seen from outside. */
  extractTriangles(minWeight) {
    const total = this.countTriangles(minWeight), room = Math.max(total, 1);
    const pos = this.device.createBuffer({ size: 36 * room }), keys = this.device.createBuffer({ size: 24 * room });
    const cols = this.colour ? this.device.createBuffer({ size: 12 * room }) : null;
    try {
      addon.tsdfVolumeEmitTriangles(this.handle, pos.ptr, keys.ptr, cols ? cols.ptr : null, total);
      const bytes = (b, n) => (n ? this.device.readBuffer(b, n) : new ArrayBuffer(0));
      return { positions: new Float32Array(bytes(pos, 36 * total)), keys: new BigUint64Array(bytes(keys, 24 * total)),
        colours: cols ? new Uint8Array(bytes(cols, 12 * total)) : null, count: total };
    } finally { pos.destroy(); keys.destroy(); if (cols) cols.destroy(); }
  }
  /** extractTriangles without the read-back: { positions, keys, colours | null, numTriangles }, the three as HipBuffers the caller destroys
   *  (f32[F][3][3], u64[F][3], rgba8[F][3]): what weldTrianglesDevice takes. */
  extractTriangleBuffers(minWeight) {
    const total = this.countTriangles(minWeight), room = Math.max(total, 1);
    const out = { positions: this.device.createBuffer({ size: 36 * room }), keys: this.device.createBuffer({ size: 24 * room }),
      colours: this.colour ? this.device.createBuffer({ size: 12 * room }) : null, numTriangles: total };
    try {
      addon.tsdfVolumeEmitTriangles(this.handle, out.positions.ptr, out.keys.ptr, out.colours ? out.colours.ptr : null, total);
    } catch (e) { destroyBuffers(out); throw e; }
    return out;
  }
  /** The welded mesh.  options.weld: 'host' (default: weldTriangles of extractTriangles) or 'device' (the triangles stay on the device and
   *  weldTrianglesDevice welds them there: the same bytes, and only the V- and F-sized arrays of the result cross the bus).  options.smooth: an iteration
   *  count (DESIGN.md section 19): the welded mesh goes through smoothMesh with its defaults -- before it is simplified -- and stats is added;
   *  options.normals: normals Float32Array[V*3], vertexNormals of the final mesh, is added; with weld 'device' the positions stay on the device through
   *  both.  options.simplify: a cell size (DESIGN.md section 18): the welded mesh goes through simplifyMesh on the grid of that cell size from the
   *  volume's origin and its object is returned; with weld 'device' the welded mesh stays on the device until it is simplified.  Without the three nothing
   *  more is launched. */
  extractMesh(minWeight, options) {
    const weld = (options && options.weld) || 'host';
    const simplify = options && options.simplify !== undefined && options.simplify !== null ? options.simplify : null;
    const smooth = options && options.smooth !== undefined && options.smooth !== null ? options.smooth : null;
    const normals = !!(options && options.normals), plain = smooth === null && !normals;
    if (weld !== 'host' && weld !== 'device') throw new Error(`extractMesh: weld must be 'host' or 'device', not ${weld}`);
    if (weld === 'host') {
      const mesh = weldTriangles(this.extractTriangles(minWeight));
      if (plain) return simplify === null ? mesh : simplifyMesh(this.device, mesh, simplify, { origin: this.origin });
      return finishMesh(this.device, mesh, this.origin, smooth, simplify, normals);
    }
    const tri = this.extractTriangleBuffers(minWeight);
    let welded = {};
    try {
      if (simplify === null && plain) return weldTrianglesDevice(this.device, tri);
      welded = weldTrianglesDevice(this.device, tri, { asBuffers: true });
      if (plain) return simplifyMesh(this.device, welded, simplify, { origin: this.origin });
      return finishMesh(this.device, welded, this.origin, smooth, simplify, normals, readWelded);
    } finally { destroyBuffers(tri); destroyBuffers(welded); }
  }
  destroy() {
    if (this.destroyed) return;
    this.destroyed = true;
    addon.tsdfVolumeDestroy(this.handle);
    this.handle = null;
  }
}
/** extractTriangles' output as an indexed mesh: { vertices: Float32Array[V*3], faces: Uint32Array[F*3], colours: Uint8Array[V*3] | null,
 *  keys: BigUint64Array[V] }.  Vertices are the triangles' distinct edge keys in ascending order (equal keys carry equal position bits); triangles are kept
 *  as emitted, zero-area ones included.  Host side. */
function weldTriangles(tri) {
  const n = tri.keys.length;
  const order = Array.from({ length: n }, (_, i) => i).sort((a, b) => (tri.keys[a] < tri.keys[b] ? -1 : (tri.keys[a] > tri.keys[b] ? 1 : a - b)));
  const faces = new Uint32Array(n), first = [];
  for (let r = 0; r < n; r++) {
    const i = order[r];
    if (r === 0 || tri.keys[i] !== tri.keys[order[r - 1]]) first.push(i);   // (the sort is stable in the index: the first occurrence, as np.unique's)
    faces[i] = first.length - 1;
  }
  const V = first.length, vertices = new Float32Array(3 * V), keys = new BigUint64Array(V), colours = tri.colours ? new Uint8Array(3 * V) : null;
  first.forEach((i, v) => {
    keys[v] = tri.keys[i];
    for (let a = 0; a < 3; a++) vertices[3 * v + a] = tri.positions[3 * i + a];
    if (colours) for (let a = 0; a < 3; a++) colours[3 * v + a] = tri.colours[4 * i + a];
  });
  return { vertices, faces, colours, keys };
}

// ---------------------------------------------------------------- welding on the device (include/webdgs.h, DESIGN.md section 17; no reference counterpart)
/** Destroys every HipBuffer among the values of `buffers` (what extractTriangleBuffers and weldTrianglesDevice hand out). */
function destroyBuffers(buffers) { Object.values(buffers).forEach((b) => { if (b instanceof HipBuffer) b.destroy(); }); }
/** A buffer the library owns whose size is exactly `size` bytes, 0 included (asDevice counts whole rows of it). */
function exactBuffer(device, size) {
  const b = addon.bufferCreate(device.handle, Math.max(size, 8));
  return new HipBuffer(device, b.ptr, size, b.handle);
}
/** The rgb bytes of `count` rgba8 words of a device buffer. */
function readRGB(device, buffer, count) {
  const rgba = new Uint8Array(count ? device.readBuffer(buffer, 4 * count) : new ArrayBuffer(0)), rgb = new Uint8Array(3 * count);
  for (let v = 0; v < count; v++) for (let a = 0; a < 3; a++) rgb[3 * v + a] = rgba[4 * v + a];
  return rgb;
}
/** The welded mesh weldTrianglesDevice hands out with asBuffers, read back: { vertices, faces, colours: rgb | null, keys }. */
function readWelded(device, b) {
  const V = b.numVertices, F = b.numFaces, bytes = (x, n) => (n ? device.readBuffer(x, n) : new ArrayBuffer(0));
  return { vertices: new Float32Array(bytes(b.vertices, 12 * V)), faces: new Uint32Array(bytes(b.faces, 12 * F)), colours: b.colours ? readRGB(device, b.colours, V) : null,
    keys: new BigUint64Array(bytes(b.keys, 8 * V)) };
}
/** Welds a triangle soup on the device (wdgs_mesh_welder): count sorts the (key, slot) pairs with a stable radix sort, flags the first pair of every
 *  distinct key and returns their number (one wait); emit writes the indexed mesh.  weldTrianglesDevice is the one-call form. */
class MeshWelder {
  constructor(device) { this.device = device; this.destroyed = false; this.numSlots = 0; this.numVertices = 0; this.handle = addon.meshWelderCreate(device.handle); }
  /** The number of distinct keys among keys u64[numSlots], numSlots three per triangle and below 2^32 (sort, flags, scan; waits once). */
  count(keys, numSlots) {
    if (keys && numSlots < 2 ** 32 && keys.size < 8 * numSlots) throw new Error('MeshWelder.count: buffer too small for the keys');
    this.numVertices = addon.meshWelderCount(this.handle, keys ? keys.ptr : null, numSlots);
    this.numSlots = numSlots;
    return this.numVertices;
  }
  /** Writes facesOut u32[numSlots], verticesOut f32[V][3] gathered from positions, coloursOut rgba8[V] gathered from colours and keysOut u64[V] for the
   *  count before it (WDGS_E_STATE otherwise; WDGS_E_CAPACITY, with nothing written, when there is room for fewer than V vertices).  Each pair and
   *  keysOut nullable.  Stream-ordered: it waits for nothing and records. */
  emit(keys, numSlots, positions, colours, facesOut, verticesOut, coloursOut, keysOut, capacity) {
    const outs = [[verticesOut, 12], [coloursOut, 4], [keysOut, 8]].filter(([b]) => b);
    const cap = capacity === undefined || capacity === null ? Math.min(0xFFFFFFFF, ...outs.map(([b, s]) => Math.floor(b.size / s))) : capacity;
    for (const [b, s] of outs) if (cap * s > b.size) throw new Error('MeshWelder.emit: the capacity exceeds the buffers');
    if (numSlots < 2 ** 32 && ((facesOut && facesOut.size < 4 * numSlots) || (positions && positions.size < 12 * numSlots) || (colours && colours.size < 4 * numSlots))) {
      throw new Error('MeshWelder.emit: buffers too small for the slots');
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshWelderEmit(this.handle, ptr(keys), numSlots, ptr(positions), ptr(colours), ptr(keysOut), ptr(verticesOut), ptr(coloursOut), ptr(facesOut), cap);
  }
  /** The last count: { passesRun, passesSkipped, vertices, slots } -- of the eight radix passes, those whose digit differs somewhere ran. */
  stats() {
    const r = addon.meshWelderStats(this.handle);
    return { passesRun: r[0], passesSkipped: r[1], vertices: r[2], slots: r[3] };
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshWelderDestroy(this.handle); this.handle = null; }
}
/** weldTriangles on the device, byte for byte: `tri` is extractTriangles' output (uploaded) or extractTriangleBuffers' (left as it is); returns what
 *  weldTriangles returns.  A vertex takes the position and colour of the lowest slot that carries its key.  options.asBuffers: vertices f32[V][3], faces
 *  u32[F][3], keys u64[V] and colours rgba8[V] (or null) stay on the device as HipBuffers of exactly those sizes -- what meshComponents,
 *  removeSmallComponents and sampleMesh take -- with numVertices and numFaces; the caller destroys them (destroyBuffers). */
function weldTrianglesDevice(device, tri, options) {
  const own = !(tri.keys instanceof HipBuffer);
  let src, F;
  if (own) {
    if (tri.keys.length % 3 !== 0) throw new Error('weldTrianglesDevice: the keys are not three per triangle');
    F = tri.keys.length / 3;
    if (tri.positions.length !== 9 * F || (tri.colours && tri.colours.length !== 12 * F)) throw new Error('weldTrianglesDevice: positions or colours disagree with the keys');
    const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); return b; };
    src = { keys: upload(tri.keys), positions: upload(tri.positions), colours: tri.colours ? upload(tri.colours) : null };
  } else {
    F = tri.numTriangles;
    src = { keys: tri.keys, positions: tri.positions, colours: tri.colours || null };
  }
  const S = 3 * F, welder = new MeshWelder(device);
  let out = {};
  try {
    const V = welder.count(src.keys, S);
    out = { vertices: exactBuffer(device, 12 * V), faces: exactBuffer(device, 4 * S), colours: src.colours ? exactBuffer(device, 4 * V) : null, keys: exactBuffer(device, 8 * V) };
    welder.emit(src.keys, S, src.positions, src.colours, out.faces, out.vertices, out.colours, out.keys, V);
    if (options && options.asBuffers) {
      device.synchronize();   // (an uploaded soup is released below)
      const result = Object.assign({}, out, { numVertices: V, numFaces: F });
      out = {};
      return result;
    }
    return readWelded(device, Object.assign({}, out, { numVertices: V, numFaces: F }));
  } finally {
    welder.destroy();
    destroyBuffers(out);
    if (own) destroyBuffers(src);
  }
}

// ---------------------------------------------------------------- simplification by vertex clustering (include/webdgs.h, DESIGN.md section 18; no reference counterpart)
/** Simplifies an indexed mesh on the device by vertex clustering (wdgs_mesh_simplifier): count keys every vertex by its cell of the grid (origin, cellSize),
 *  numbers the clusters, reduces each to one representative, drops the faces that are invalid, outside, collapsed or duplicates and returns
 *  { vertices: V', faces: F' } (one wait); emit writes the simplified mesh.  simplifyMesh is the one-call form. */
class MeshSimplifier {
  constructor(device) { this.device = device; this.destroyed = false; this.numVertices = 0; this.numFaces = 0; this.handle = addon.meshSimplifierCreate(device.handle); }
  /** { vertices, faces }: V' and F' for vertices f32[numVertices][3], faces u32[numFaces][3] and (nullable) colours rgba8[numVertices]; origin: three numbers. */
  count(vertices, numVertices, faces, numFaces, colours, origin, cellSize) {
    if (numVertices < 2 ** 31 && numFaces < 2 ** 31 && ((vertices && vertices.size < 12 * numVertices) || (faces && faces.size < 12 * numFaces) ||
      (colours && colours.size < 4 * numVertices))) throw new Error('MeshSimplifier.count: buffers too small for the mesh');
    const ptr = (b) => (b ? b.ptr : null);
    const r = addon.meshSimplifierCount(this.handle, ptr(vertices), numVertices, ptr(faces), numFaces, ptr(colours), Math.fround(origin[0]), Math.fround(origin[1]),
      Math.fround(origin[2]), Math.fround(cellSize));
    this.numVertices = r[0]; this.numFaces = r[1];
    return { vertices: r[0], faces: r[1] };
  }
  /** Writes verticesOut f32[V'][3], facesOut u32[F'][3], coloursOut rgba8[V'] (with colours), keysOut u64[V'], faceMap u32[F'] and vertexCluster
   *  u32[numVertices] (the last three nullable) for the count before it (WDGS_E_STATE otherwise; WDGS_E_CAPACITY, with nothing written, when there is room
   *  for fewer than V' vertices or F' faces).  Stream-ordered: it waits for nothing and records. */
  emit(vertices, numVertices, faces, numFaces, colours, verticesOut, facesOut, coloursOut, keysOut, faceMap, vertexCluster, capacityVertices, capacityFaces) {
    const room = (pairs) => Math.min(0xFFFFFFFF, ...pairs.filter(([b]) => b).map(([b, s]) => Math.floor(b.size / s)));
    const vouts = [[verticesOut, 12], [coloursOut, 4], [keysOut, 8]], fouts = [[facesOut, 12], [faceMap, 4]];
    const cv = capacityVertices === undefined || capacityVertices === null ? room(vouts) : capacityVertices;
    const cf = capacityFaces === undefined || capacityFaces === null ? room(fouts) : capacityFaces;
    for (const [b, s] of vouts) if (b && cv * s > b.size) throw new Error('MeshSimplifier.emit: the capacity exceeds the buffers');
    for (const [b, s] of fouts) if (b && cf * s > b.size) throw new Error('MeshSimplifier.emit: the capacity exceeds the buffers');
    if (vertexCluster && vertexCluster.size < 4 * numVertices) throw new Error('MeshSimplifier.emit: vertexCluster is too small for the vertices');
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshSimplifierEmit(this.handle, ptr(vertices), numVertices, ptr(faces), numFaces, ptr(colours), ptr(verticesOut), ptr(coloursOut), ptr(keysOut), ptr(facesOut),
      ptr(faceMap), ptr(vertexCluster), cv, cf);
  }
  /** The last count: { clusters, invalid, outside, collapsed, duplicate, vertices, faces } -- the occupied cells, the dropped faces by class, V' and F'. */
  stats() {
    const r = addon.meshSimplifierStats(this.handle);
    return { clusters: r[0], invalid: r[1], outside: r[2], collapsed: r[3], duplicate: r[4], vertices: r[5], faces: r[6] };
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshSimplifierDestroy(this.handle); this.handle = null; }
}
/** `mesh` simplified by vertex clustering on a grid of cellSize from options.origin: the vertices of one cell become one vertex at the integer mean of their
 *  sub-cell offsets (colours alike), faces that collapse or repeat a lower face's cluster triple are dropped, unreferenced clusters are left out.  `mesh` is
 *  what extractMesh / loadMeshPLY return (uploaded; colours Uint8Array[V*3] get an alpha of 255, [V*4] go as they are) or { vertices, faces, colours | null }
 *  as HipBuffers (f32[V][3], u32[F][3], rgba8[V]) with numVertices / numFaces or whole buffers, as weldTrianglesDevice hands out with asBuffers (left as it
 *  is).  options.origin: three numbers; without one, the per-axis minimum of the finite vertices (typed-array input only; a device mesh needs one).  Returns
 *  { vertices, faces, colours | null, keys, faceMap, vertexCluster, stats }; a function of its arguments alone, bit for bit (include/webdgs.h states it).
 *  options.asBuffers: the six stay on the device as HipBuffers of exactly their sizes (colours rgba8[V']), with numVertices and numFaces. */
function simplifyMesh(device, mesh, cellSize, options) {
  const o = options || {}, own = !(mesh.vertices instanceof HipBuffer);
  let src, V, F, origin = o.origin;
  if (own) {
    if (mesh.vertices.length % 3 !== 0 || mesh.faces.length % 3 !== 0) throw new Error('simplifyMesh: vertices and faces are three values per row');
    V = mesh.vertices.length / 3; F = mesh.faces.length / 3;
    let rgba = null;
    if (mesh.colours) {
      if (mesh.colours.length === 4 * V) rgba = mesh.colours;
      else if (mesh.colours.length === 3 * V) {
        rgba = new Uint8Array(4 * V).fill(255);
        for (let v = 0; v < V; v++) for (let a = 0; a < 3; a++) rgba[4 * v + a] = mesh.colours[3 * v + a];
      } else throw new Error(`simplifyMesh: ${mesh.colours.length} colour bytes for ${V} vertices`);
    }
    if (origin === undefined || origin === null) {
      origin = [Infinity, Infinity, Infinity];
      for (let v = 0; v < V; v++) {
        const p = mesh.vertices.subarray(3 * v, 3 * v + 3);
        if (Number.isFinite(p[0]) && Number.isFinite(p[1]) && Number.isFinite(p[2])) for (let a = 0; a < 3; a++) origin[a] = Math.min(origin[a], p[a]);
      }
      if (!Number.isFinite(origin[0])) origin = [0, 0, 0];
    }
    const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); return b; };
    src = { vertices: upload(mesh.vertices instanceof Float32Array ? mesh.vertices : Float32Array.from(mesh.vertices)),
      faces: upload(mesh.faces instanceof Uint32Array ? mesh.faces : Uint32Array.from(mesh.faces)), colours: rgba ? upload(rgba) : null };
  } else {
    if (origin === undefined || origin === null) throw new Error('simplifyMesh: a mesh on the device needs an explicit origin');
    V = mesh.numVertices === undefined ? Math.floor(mesh.vertices.size / 12) : mesh.numVertices;
    F = mesh.numFaces === undefined ? Math.floor(mesh.faces.size / 12) : mesh.numFaces;
    src = { vertices: mesh.vertices, faces: mesh.faces, colours: mesh.colours || null };
  }
  const simplifier = new MeshSimplifier(device);
  let out = {};
  try {
    const n = simplifier.count(src.vertices, V, src.faces, F, src.colours, origin, cellSize), nv = n.vertices, nf = n.faces;
    out = { vertices: exactBuffer(device, 12 * nv), faces: exactBuffer(device, 12 * nf), colours: src.colours ? exactBuffer(device, 4 * nv) : null,
      keys: exactBuffer(device, 8 * nv), faceMap: exactBuffer(device, 4 * nf), vertexCluster: exactBuffer(device, 4 * V) };
    simplifier.emit(src.vertices, V, src.faces, F, src.colours, out.vertices, out.faces, out.colours, out.keys, out.faceMap, out.vertexCluster, nv, nf);
    const stats = simplifier.stats();
    if (o.asBuffers) {
      device.synchronize();   // (an uploaded mesh is released below)
      const result = Object.assign({}, out, { numVertices: nv, numFaces: nf, stats });
      out = {};
      return result;
    }
    return readSimplified(device, Object.assign({}, out, { numVertices: nv, numFaces: nf, stats }), V);
  } finally {
    simplifier.destroy();
    destroyBuffers(out);
    if (own) destroyBuffers(src);
  }
}

/** The mesh simplifyMesh hands out with asBuffers for an input of V vertices, read back as simplifyMesh returns it. */
function readSimplified(device, b, V) {
  const nv = b.numVertices, nf = b.numFaces, bytes = (x, k) => (k ? device.readBuffer(x, k) : new ArrayBuffer(0));
  return { vertices: new Float32Array(bytes(b.vertices, 12 * nv)), faces: new Uint32Array(bytes(b.faces, 12 * nf)), colours: b.colours ? readRGB(device, b.colours, nv) : null,
    keys: new BigUint64Array(bytes(b.keys, 8 * nv)), faceMap: new Uint32Array(bytes(b.faceMap, 4 * nf)), vertexCluster: new Uint32Array(bytes(b.vertexCluster, 4 * V)),
    stats: b.stats };
}

// ---------------------------------------------------------------- adjacency, smoothing and vertex normals (include/webdgs.h, DESIGN.md section 19; no reference counterpart)
const SMOOTH_PIN_BOUNDARY = 1;   // WDGS_SMOOTH_PIN_BOUNDARY
const ADJACENCY_STATS = ['directedEdges', 'edges', 'boundaryEdges', 'nonManifoldEdges', 'invalidFaces', 'boundaryVertices', 'isolatedVertices', 'maxDegree'];
/** The per-vertex neighbour lists of an indexed mesh on the device (wdgs_mesh_adjacency) and what stands on them: count sorts the faces' directed half-edge
 *  keys (the welder's stable u64 sort over 6 F slots), delimits the rows, flags the boundary and returns E (one wait); emit writes rowStart, neighbours and
 *  boundary; smooth runs Taubin's lambda | mu steps and normals the area-weighted vertex normals over that count, both stream-ordered.  meshAdjacency,
 *  smoothMesh and vertexNormals are the one-call forms. */
class MeshAdjacency {
  constructor(device) {
    this.device = device; this.destroyed = false; this.numEdges = 0; this.numVertices = 0; this.numFaces = 0;
    this.handle = addon.meshAdjacencyCreate(device.handle);
  }
  /** E, the number of directed edges of faces u32[numFaces][3] over numVertices vertices (waits once).  The faces must stay as they are while normals may
   *  still be called. */
  count(faces, numFaces, numVertices) {
    if (6 * numFaces < 2 ** 32 && faces && faces.size < 12 * numFaces) throw new Error('MeshAdjacency.count: buffer too small for the faces');
    this.numEdges = addon.meshAdjacencyCount(this.handle, faces ? faces.ptr : null, numFaces, numVertices);
    this.numVertices = numVertices; this.numFaces = numFaces;
    return this.numEdges;
  }
  /** Writes rowStart u32[V + 1], neighbours u32[E] and boundary u32[V] of the count before it, each nullable (WDGS_E_STATE without a count;
   *  WDGS_E_CAPACITY, with nothing written, when there is room for fewer than E edges).  Stream-ordered: it waits for nothing and records. */
  emit(rowStart, neighbours, boundary, capacityEdges) {
    const cap = capacityEdges === undefined || capacityEdges === null ? (neighbours ? Math.floor(neighbours.size / 4) : 0xFFFFFFFF) : capacityEdges;
    if (neighbours && 4 * cap > neighbours.size) throw new Error('MeshAdjacency.emit: the capacity exceeds the buffer');
    if ((rowStart && rowStart.size < 4 * (this.numVertices + 1)) || (boundary && boundary.size < 4 * this.numVertices)) {
      throw new Error('MeshAdjacency.emit: buffers too small for the vertices');
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshAdjacencyEmit(this.handle, ptr(rowStart), ptr(neighbours), ptr(boundary), cap);
  }
  /** verticesOut f32[V][3] = verticesIn after `iterations` rounds of step(lambda) then step(mu) over the counted adjacency (a weight of exactly 0 skips its
   *  step; verticesOut may be verticesIn).  options: { lambda = 0.5, mu = -0.53, pinBoundary = true }.  WDGS_E_STATE unless numVertices is the count's.
   *  Stream-ordered: it waits for nothing, allocates nothing and records. */
  smooth(verticesIn, verticesOut, numVertices, iterations, options) {
    const o = options || {}, lambda = o.lambda === undefined ? 0.5 : o.lambda, mu = o.mu === undefined ? -0.53 : o.mu, pin = o.pinBoundary === undefined ? true : o.pinBoundary;
    for (const b of [verticesIn, verticesOut]) if (b && numVertices === this.numVertices && b.size < 12 * numVertices) throw new Error('MeshAdjacency.smooth: buffer too small for the vertices');
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshAdjacencySmooth(this.handle, ptr(verticesIn), ptr(verticesOut), numVertices, iterations === undefined || iterations === null ? 10 : iterations,
      Math.fround(lambda), Math.fround(mu), pin ? SMOOTH_PIN_BOUNDARY : 0);
  }
  /** normalsOut f32[V][3]: the area-weighted normals of vertices f32[V][3] over the counted faces -- `faces` must be the buffer that was counted, unchanged
   *  (WDGS_E_STATE otherwise).  Stream-ordered: it waits for nothing and records. */
  normals(vertices, faces, numVertices, numFaces, normalsOut) {
    for (const b of [vertices, normalsOut]) if (b && numVertices === this.numVertices && b.size < 12 * numVertices) throw new Error('MeshAdjacency.normals: buffer too small for the vertices');
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshAdjacencyNormals(this.handle, ptr(vertices), ptr(faces), numVertices, numFaces, ptr(normalsOut));
  }
  /** The last count: { directedEdges, edges, boundaryEdges, nonManifoldEdges, invalidFaces, boundaryVertices, isolatedVertices, maxDegree }. */
  stats() {
    const r = addon.meshAdjacencyStats(this.handle), out = {};
    ADJACENCY_STATS.forEach((k, i) => { out[k] = r[i]; });
    return out;
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshAdjacencyDestroy(this.handle); this.handle = null; }
}
/** { vertices, faces, V, F, own }: the mesh's positions and faces as HipBuffers -- uploaded from typed arrays (own: the caller destroys them) or taken as they
 *  are from an object of buffers with numVertices / numFaces or whole buffers. */
function meshOnDevice(device, mesh, what) {
  if (!(mesh.vertices instanceof HipBuffer)) {
    if (mesh.vertices.length % 3 !== 0 || mesh.faces.length % 3 !== 0) throw new Error(`${what}: vertices and faces are three values per row`);
    const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); return b; };
    return { vertices: upload(mesh.vertices instanceof Float32Array ? mesh.vertices : Float32Array.from(mesh.vertices)),
      faces: upload(mesh.faces instanceof Uint32Array ? mesh.faces : Uint32Array.from(mesh.faces)), V: mesh.vertices.length / 3, F: mesh.faces.length / 3, own: true };
  }
  if (!(mesh.faces instanceof HipBuffer)) throw new Error(`${what}: vertices on the device need faces on the device`);
  return { vertices: mesh.vertices, faces: mesh.faces, V: mesh.numVertices === undefined ? Math.floor(mesh.vertices.size / 12) : mesh.numVertices,
    F: mesh.numFaces === undefined ? Math.floor(mesh.faces.size / 12) : mesh.numFaces, own: false };
}
/** The neighbour lists of `mesh` (typed arrays or device buffers; only the faces and the vertex count matter): { rowStart: Uint32Array[V+1], neighbours:
 *  Uint32Array[E], boundary: Uint32Array[V], stats } -- vertex v neighbours neighbours[rowStart[v] .. rowStart[v+1]), ascending; boundary is 1 on both ends
 *  of every edge that one face alone holds.  A function of the faces alone, bit for bit (include/webdgs.h states it). */
function meshAdjacency(device, mesh) {
  const src = meshOnDevice(device, mesh, 'meshAdjacency'), adjacency = new MeshAdjacency(device);
  let out = {};
  try {
    const V = src.V, E = adjacency.count(src.faces, src.F, V);
    out = { rowStart: exactBuffer(device, 4 * (V + 1)), neighbours: exactBuffer(device, 4 * E), boundary: exactBuffer(device, 4 * V) };
    adjacency.emit(out.rowStart, out.neighbours, out.boundary, E);
    const bytes = (b, n) => (n ? device.readBuffer(b, n) : new ArrayBuffer(0));
    return { rowStart: new Uint32Array(bytes(out.rowStart, 4 * (V + 1))), neighbours: new Uint32Array(bytes(out.neighbours, 4 * E)),
      boundary: new Uint32Array(bytes(out.boundary, 4 * V)), stats: adjacency.stats() };
  } finally {
    adjacency.destroy();
    destroyBuffers(out);
    if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
  }
}
/** { smoothed, normals, stats } of a mesh on the device through one MeshAdjacency: a new buffer of the positions after `smooth` iterations (null: not
 *  wanted) and a new buffer of the normals of the smoothed -- else the given -- positions.  The caller destroys both. */
function smoothAndNormals(device, vertices, faces, V, F, smooth, normals, options) {
  const adjacency = new MeshAdjacency(device);
  let out = {};
  try {
    adjacency.count(faces, F, V);
    if (smooth !== null) {
      out.smoothed = exactBuffer(device, 12 * V);
      adjacency.smooth(vertices, out.smoothed, V, smooth, options);
    }
    if (normals) {
      out.normals = exactBuffer(device, 12 * V);
      adjacency.normals(out.smoothed || vertices, faces, V, F, out.normals);
    }
    const result = { smoothed: out.smoothed || null, normals: out.normals || null, stats: adjacency.stats() };
    device.synchronize();   // (the object's arrays are released below)
    out = {};
    return result;
  } finally {
    adjacency.destroy();
    destroyBuffers(out);
  }
}
/** `mesh` after `iterations` (default 10) rounds of Taubin's lambda | mu smoothing (mu = 0: plain Laplacian smoothing): every vertex moves towards, then away
 *  from, the f32 mean of its neighbours, summed in ascending neighbour order; with pinBoundary the ends of boundary edges stay where they are.  options:
 *  { lambda = 0.5, mu = -0.53, pinBoundary = true, asBuffers }.  `mesh` is what extractMesh / loadMeshPLY return, or an object of HipBuffers as
 *  weldTrianglesDevice and simplifyMesh hand out with asBuffers (left as it is).  Returns the mesh's object with new vertices, every other entry passed through,
 *  and stats added; bit for bit a function of its arguments (include/webdgs.h states it).  options.asBuffers: vertices is a new HipBuffer f32[V][3] the
 *  caller destroys; a typed-array mesh's faces are then handed out as a buffer too, with numVertices and numFaces. */
function smoothMesh(device, mesh, iterations, options) {
  const o = options || {}, src = meshOnDevice(device, mesh, 'smoothMesh');
  let smoothed = null, keepFaces = false;
  try {
    const r = smoothAndNormals(device, src.vertices, src.faces, src.V, src.F, iterations === undefined || iterations === null ? 10 : iterations, false, o);
    smoothed = r.smoothed;
    if (o.asBuffers) {
      const result = Object.assign({}, mesh, { vertices: smoothed, stats: r.stats, numVertices: src.V, numFaces: src.F });
      if (src.own) { result.faces = src.faces; keepFaces = true; }
      smoothed = null;
      return result;
    }
    return Object.assign({}, mesh, { vertices: new Float32Array(src.V ? device.readBuffer(smoothed, 12 * src.V) : new ArrayBuffer(0)), stats: r.stats });
  } finally {
    if (smoothed) smoothed.destroy();
    if (src.own) { src.vertices.destroy(); if (!keepFaces) src.faces.destroy(); }
  }
}
/** The area-weighted unit normals Float32Array[V*3] of `mesh` (typed arrays or device buffers): per vertex the sum of its faces' cross products in the order
 *  the half-edge sort fixes, normalised; (0, 0, 0) for a vertex without a face of non-zero finite area. */
function vertexNormals(device, mesh) {
  const src = meshOnDevice(device, mesh, 'vertexNormals');
  let normals = null;
  try {
    normals = smoothAndNormals(device, src.vertices, src.faces, src.V, src.F, null, true).normals;
    return new Float32Array(src.V ? device.readBuffer(normals, 12 * src.V) : new ArrayBuffer(0));
  } finally {
    if (normals) normals.destroy();
    if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
  }
}
/** What extractMesh does to a welded (and compacted) mesh, in its order: smoothMesh(mesh, smooth) when smooth is not null, then simplifyMesh(mesh, simplify,
 *  origin) when simplify is not null, then normals = vertexNormals(mesh) when asked for; returned as typed arrays.  A typed-array mesh goes through the three
 *  functions as they are.  A mesh of HipBuffers with numVertices and numFaces stays on the device throughout: its vertices buffer is replaced by the smoothed
 *  one (the caller still destroys the object), and read(device, mesh) turns it into the object to return when it is not simplified. */
function finishMesh(device, mesh, origin, smooth, simplify, normals, read) {
  if (!(mesh.vertices instanceof HipBuffer)) {
    if (smooth !== null) mesh = smoothMesh(device, mesh, smooth);
    if (simplify !== null) mesh = simplifyMesh(device, mesh, simplify, { origin });
    return normals ? Object.assign({}, mesh, { normals: vertexNormals(device, mesh) }) : mesh;
  }
  const V = mesh.numVertices, F = mesh.numFaces;
  const normalsOf = (buf, n) => { try { return new Float32Array(n ? device.readBuffer(buf, 12 * n) : new ArrayBuffer(0)); } finally { buf.destroy(); } };
  let stats = null, vn = null;
  if (smooth !== null || (normals && simplify === null)) {
    const r = smoothAndNormals(device, mesh.vertices, mesh.faces, V, F, smooth, normals && simplify === null);
    stats = r.stats;
    if (r.smoothed) { mesh.vertices.destroy(); mesh.vertices = r.smoothed; }
    if (r.normals) vn = normalsOf(r.normals, V);
  }
  if (simplify === null) {
    const out = read(device, mesh);
    if (smooth !== null) out.stats = stats;
    if (normals) out.normals = vn;
    return out;
  }
  if (!normals) return simplifyMesh(device, mesh, simplify, { origin });
  const simplified = simplifyMesh(device, mesh, simplify, { origin, asBuffers: true });
  try {
    const out = readSimplified(device, simplified, V);
    out.normals = normalsOf(smoothAndNormals(device, simplified.vertices, simplified.faces, simplified.numVertices, simplified.numFaces, null, true).normals, simplified.numVertices);
    return out;
  } finally { destroyBuffers(simplified); }
}

// ---------------------------------------------------------------- mesh rasterization and depth agreement (include/webdgs.h, DESIGN.md section 20; no reference counterpart)
const CULL_MODES = { none: 0, back: 1, front: 2 };   // WDGS_CULL_NONE, WDGS_CULL_BACK, WDGS_CULL_FRONT
const MESH_RASTER_LARGE_FACE_PIXELS = 8;             // WDGS_MESH_RASTER_LARGE_FACE_PIXELS
const MESH_RASTER_MAX_SIZE = 8192;                   // WDGS_MESH_RASTER_MAX_SIZE
const MESH_RASTER_NEAR = 0.01;   // the depth below which the forward pass drops a Gaussian (csrc/project.hip, project_one: ndc.z < 0 under the cameras' znear of 0.01)
const NO_FACE = 0xFFFFFFFF;
const RASTER_STATS = ['invalidFaces', 'clippedFaces', 'degenerateFaces', 'culledFaces', 'emptyFaces', 'rasterizedFaces', 'coveredPixels', 'viewportMismatch'];
const RASTER_OUTPUTS = { depth: [4, Float32Array], face: [4, Uint32Array], colour: [4, Uint8Array], normal: [16, Float32Array] };   // bytes per pixel, read-back type
/** A z-buffered triangle rasterizer under the library's camera block (wdgs_mesh_rasterizer): encode draws an indexed mesh on the device into the depth, face,
 *  colour and normal images asked for, stats reads the face classes and the covered pixels of the last encode.  Every byte is a function of the input alone
 *  (include/webdgs.h states the definition).  There is no clipping: a face with a vertex nearer than `near` is dropped whole.  rasterizeMesh is the one-call form. */
class MeshRasterizer {
  constructor(device) { this.device = device; this.destroyed = false; this.handle = addon.meshRasterizerCreate(device.handle); }
  /** Draws vertices f32[numVertices][3], faces u32[numFaces][3] (and colours rgba8[numVertices] for a colour image) under `camera` (the 68-float block on the
   *  device) into options.depth f32, .face u32, .colour rgba8 and .normal rgba32f images of width x height, each optional; options.near (default
   *  MESH_RASTER_NEAR), options.cull ('none', 'back', 'front').  Stream-ordered: it waits for nothing and records -- except a call that has to grow the object's
   *  arrays (WDGS_E_STATE while recording; encode once eagerly first). */
  encode(vertices, numVertices, faces, numFaces, colours, camera, width, height, options) {
    const o = options || {}, cull = o.cull || 'none', near = o.near === undefined || o.near === null ? MESH_RASTER_NEAR : o.near;
    if (!(cull in CULL_MODES)) { const e = new Error(`MeshRasterizer.encode: unknown cull mode ${cull} (none, back, front)`); e.code = 'WDGS_E'; throw e; }
    if (numVertices < 2 ** 31 && 3 * numFaces < 2 ** 32 && ((vertices && vertices.size < 12 * numVertices) || (faces && faces.size < 12 * numFaces) ||
                                                           (colours && colours.size < 4 * numVertices))) throw new Error('MeshRasterizer.encode: buffers too small for the mesh');
    if (camera.size < 272) throw new Error('MeshRasterizer.encode: the camera block has 68 floats');
    if (width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE) {
      for (const k of Object.keys(RASTER_OUTPUTS)) if (o[k] && o[k].size < RASTER_OUTPUTS[k][0] * width * height) throw new Error(`MeshRasterizer.encode: the ${k} image is too small for ${width}x${height}`);
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshRasterizerEncode(this.handle, ptr(vertices), numVertices, ptr(faces), numFaces, ptr(colours), camera.ptr, width, height, Math.fround(near), CULL_MODES[cull],
      ptr(o.depth), ptr(o.face), ptr(o.colour), ptr(o.normal));
  }
  /** The last encode: { invalidFaces, clippedFaces, degenerateFaces, culledFaces, emptyFaces, rasterizedFaces, coveredPixels, viewportMismatch } -- every face
   *  is in exactly one class.  Waits (WDGS_E_STATE before an encode and while recording). */
  stats() {
    const r = addon.meshRasterizerStats(this.handle), out = {};
    RASTER_STATS.forEach((k, i) => { out[k] = r[i]; });
    return out;
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshRasterizerDestroy(this.handle); this.handle = null; }
}
/** The images of `mesh` under `camera` (the 68-float block: a Float32Array or a HipBuffer): { depth: Float32Array[H*W], face: Uint32Array[H*W], colour:
 *  Uint8Array[H*W*4], normal: Float32Array[H*W*4], stats } with the options.outputs asked for (default ['depth', 'face']).  `mesh` is what extractMesh /
 *  loadMeshPLY return, or an object of HipBuffers as weldTrianglesDevice and simplifyMesh hand out with asBuffers (left as it is); 'colour' needs its colours.
 *  A pixel no face covers has depth 0, face NO_FACE, colour and normal all zero.  options: { near = MESH_RASTER_NEAR, cull = 'none', outputs, asBuffers }.
 *  A function of its arguments alone, bit for bit (include/webdgs.h states it).  options.asBuffers: the images stay on the device as HipBuffers the caller
 *  destroys. */
function rasterizeMesh(device, mesh, camera, width, height, options) {
  const o = options || {}, outputs = o.outputs || ['depth', 'face'];
  for (const k of outputs) if (!(k in RASTER_OUTPUTS)) throw new Error(`rasterizeMesh: unknown output ${k} (depth, face, colour, normal)`);
  const src = meshOnDevice(device, mesh, 'rasterizeMesh');
  const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); return b; };
  let colours = null, ownColours = false, cam = null, ownCam = false, rasterizer = null, out = {};
  try {
    if (outputs.includes('colour')) {
      const c = mesh.colours;
      if (!c) { const e = new Error('rasterizeMesh: a colour image needs a mesh with colours'); e.code = 'WDGS_E'; throw e; }
      if (c instanceof HipBuffer) colours = c;
      else {
        let rgba = c;
        if (c.length === 3 * src.V) {
          rgba = new Uint8Array(4 * src.V).fill(255);
          for (let v = 0; v < src.V; v++) for (let a = 0; a < 3; a++) rgba[4 * v + a] = c[3 * v + a];
        } else if (c.length !== 4 * src.V) throw new Error(`rasterizeMesh: ${c.length} colour bytes for ${src.V} vertices`);
        colours = upload(rgba instanceof Uint8Array ? rgba : Uint8Array.from(rgba)); ownColours = true;
      }
    }
    if (camera instanceof HipBuffer) cam = camera;
    else {
      if (camera.length !== 68) throw new Error(`rasterizeMesh: the camera block has 68 floats, got ${camera.length}`);
      cam = upload(camera instanceof Float32Array ? camera : Float32Array.from(camera)); ownCam = true;
    }
    rasterizer = new MeshRasterizer(device);
    const npix = width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE ? width * height : 0;
    for (const k of outputs) out[k] = exactBuffer(device, RASTER_OUTPUTS[k][0] * npix);
    rasterizer.encode(src.vertices, src.V, src.faces, src.F, colours, cam, width, height, Object.assign({ near: o.near, cull: o.cull }, out));
    const stats = rasterizer.stats();
    if (o.asBuffers) { const result = Object.assign({}, out, { stats }); out = {}; return result; }
    const result = { stats };
    for (const k of outputs) result[k] = new RASTER_OUTPUTS[k][1](npix ? device.readBuffer(out[k], RASTER_OUTPUTS[k][0] * npix) : new ArrayBuffer(0));
    return result;
  } finally {
    if (rasterizer) rasterizer.destroy();
    destroyBuffers(out);
    if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
    if (ownColours) colours.destroy();
    if (ownCam) cam.destroy();
  }
}
/** Stream-ordered depthAgreement: the five u64 sums into the first 40 bytes of `out` (no host wait).  options: { bWeightSum, minWeightSum = 0 }. */
function encodeDepthAgreement(device, a, b, width, height, maxDifference, threshold, out, options) {
  const o = options || {}, n = width * height;
  if (a.size < 4 * n || b.size < 4 * n || (o.bWeightSum && o.bWeightSum.size < 4 * n) || out.size < 40) throw new Error(`depthAgreement: buffers too small for ${width}x${height}`);
  addon.depthAgreement(device.handle, a.ptr, b.ptr, o.bWeightSum ? o.bWeightSum.ptr : null, Math.fround(o.minWeightSum || 0), width, height, Math.fround(maxDifference),
    Math.fround(threshold), out.ptr);
}
/** The five sums as depthAgreement returns them (Numbers, exact below 2^53). */
function depthAgreementResult(sums, maxDifference) {
  const [both, onlyA, onlyB, within, sum_q] = sums.map(Number);
  return { both, onlyA, onlyB, within, sum_q, mean: both ? sum_q * Math.fround(maxDifference) / 2 ** 24 / both : NaN };
}
/** How far two f32 depth images (Float32Array or HipBuffer) agree: both, onlyA, onlyB count the pixels where both, `a` alone, `b` alone have a depth (finite
 *  and > 0; `b` also only where options.bWeightSum >= options.minWeightSum when that image is given); within those of `both` with |a - b| <= threshold; sum_q
 *  the sum of u32(min(|a - b| / maxDifference, 1) 2^24) and mean = sum_q maxDifference / 2^24 / both (NaN when both is 0).  Exact integer sums.
 *  0 < threshold <= maxDifference.  Synchronises. */
function depthAgreement(device, a, b, width, height, maxDifference, threshold, options) {
  const o = options || {}, n = width * height, owned = [];
  const onDevice = (x, what) => {
    if (!x || x instanceof HipBuffer) return x || null;
    if (x.length !== n) throw new Error(`depthAgreement: ${what} has ${x.length} values for ${width}x${height}`);
    const d = asDevice(device, x, Float32Array, 1, `depthAgreement: ${what}`);
    owned.push(d.buf);
    return d.buf;
  };
  const out = device.createBuffer({ size: 40 });
  try {
    encodeDepthAgreement(device, onDevice(a, 'a'), onDevice(b, 'b'), width, height, maxDifference, threshold, out,
      { bWeightSum: onDevice(o.bWeightSum, 'bWeightSum'), minWeightSum: o.minWeightSum });
    return depthAgreementResult([...new BigUint64Array(device.readBuffer(out, 40))], maxDifference);
  } finally { out.destroy(); owned.forEach((x) => x.destroy()); }
}

// ---------------------------------------------------------------- mesh accuracy metrics (include/webdgs.h, DESIGN.md section 14; no reference counterpart)
const NO_INDEX = 0xFFFFFFFF;
const KNN_EXCLUDE_SELF = 1;   // WDGS_KNN_EXCLUDE_SELF

/** { buf, rows, owned } of a [rows, width] array given as a typed array (uploaded; owned) or as a HipBuffer (whole rows of it). */
function asDevice(device, array, Type, width, what) {
  if (array instanceof HipBuffer) return { buf: array, rows: Math.floor(array.size / (Type.BYTES_PER_ELEMENT * width)), owned: false };
  const a = array instanceof Type ? array : Type.from(array);
  if (a.length % width !== 0) throw new Error(`${what}: expected ${width} values per row, got ${a.length} values`);
  const buf = device.createBuffer({ size: Math.max(a.byteLength, 4), label: what });
  if (a.byteLength) device.queue.writeBuffer(buf, 0, a);
  return { buf, rows: a.length / width, owned: true };
}
/** Area-weighted surface sampling of a triangle mesh on the device (wdgs_mesh_sampler): count gives every triangle its dithered share of `density`
 *  samples per unit area and returns the total (it waits), emit writes them, one thread per sample.  sampleMesh is the one-call form. */
class MeshSampler {
  constructor(device) { this.device = device; this.destroyed = false; this.handle = addon.meshSamplerCreate(device.handle); }
  count(vertices, numVertices, faces, numFaces, density, seed) {
    if (vertices.size < 12 * numVertices || faces.size < 12 * numFaces) throw new Error('MeshSampler.count: buffers too small for the mesh');
    return addon.meshSamplerCount(this.handle, vertices.ptr, numVertices, faces.ptr, numFaces, density, (seed || 0) >>> 0);
  }
  /** points f32[total][3] and face u32[total] (optional) for the arguments of the count before it (WDGS_E_STATE otherwise; WDGS_E_CAPACITY when there
   *  is too little room).  Stream-ordered. */
  emit(vertices, numVertices, faces, numFaces, density, seed, points, face, capacity) {
    const cap = capacity === undefined || capacity === null ? Math.min(Math.floor(points.size / 12), face ? Math.floor(face.size / 4) : 0xFFFFFFFF) : capacity;
    if (cap * 12 > points.size || (face && cap * 4 > face.size)) throw new Error('MeshSampler.emit: the capacity exceeds the buffers');
    addon.meshSamplerEmit(this.handle, vertices.ptr, numVertices, faces.ptr, numFaces, density, (seed || 0) >>> 0, points.ptr, face ? face.ptr : null, cap);
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshSamplerDestroy(this.handle); this.handle = null; }
}
/** Points on the surface of `mesh` ({ vertices, faces } as extractMesh returns them, or as HipBuffers), `density` per unit area on average, every triangle
 *  getting floor(area density + dither) of them: { points: Float32Array[N*3], face: Uint32Array[N], count: N }, the samples of a triangle consecutive,
 *  triangles in order; a function of its arguments alone, bit for bit.  options.asBuffers: points and face stay on the device as HipBuffers. */
function sampleMesh(device, mesh, density, seed, options) {
  const o = options || {};
  const v = asDevice(device, mesh.vertices, Float32Array, 3, 'sampleMesh: vertices'), f = asDevice(device, mesh.faces, Uint32Array, 3, 'sampleMesh: faces');
  const sampler = new MeshSampler(device);
  let points = null, face = null;
  try {
    const total = sampler.count(v.buf, v.rows, f.buf, f.rows, density, seed);
    points = device.createBuffer({ size: 12 * Math.max(total, 1), label: 'mesh samples' });
    face = device.createBuffer({ size: 4 * Math.max(total, 1), label: 'mesh sample faces' });
    sampler.emit(v.buf, v.rows, f.buf, f.rows, density, seed, points, face, total);
    if (o.asBuffers) {
      device.synchronize();   // (the uploaded mesh is released below)
      const out = { points, face, count: total };
      points = face = null;
      return out;
    }
    const bytes = (b, n) => (n ? device.readBuffer(b, n) : new ArrayBuffer(0));
    return { points: new Float32Array(bytes(points, 12 * total)), face: new Uint32Array(bytes(face, 4 * total)), count: total };
  } finally {
    sampler.destroy();
    if (v.owned) v.buf.destroy();
    if (f.owned) f.buf.destroy();
    if (points) points.destroy();
    if (face) face.destroy();
  }
}
// ---------------------------------------------------------------- mesh connected components (include/webdgs.h, DESIGN.md section 16; no reference counterpart)
/** Connected components of an indexed mesh on the device (wdgs_mesh_components): label cuts the faces into components (a lock-free union-find, one
 *  wait), select takes the components to keep, compact writes the kept part.  meshComponents and removeSmallComponents are the one-call forms. */
class MeshComponents {
  constructor(device) {
    this.device = device; this.destroyed = false; this.numFaces = 0; this.numVertices = 0; this.count = 0; this.invalidFaces = 0;
    this.handle = addon.meshComponentsCreate(device.handle);
  }
  /** Labels faces u32[numFaces][3] over numVertices vertices and returns the number of components (waits once). */
  label(faces, numFaces, numVertices) {
    if (faces && numFaces < 2 ** 31 && faces.size < 12 * numFaces) throw new Error('MeshComponents.label: buffer too small for the faces');
    const r = addon.meshComponentsLabel(this.handle, faces ? faces.ptr : null, numFaces, numVertices);
    this.numFaces = numFaces; this.numVertices = numVertices; this.count = r[0]; this.invalidFaces = r[1];
    return this.count;
  }
  /** The last labelling: { count, faceComponent: Uint32Array[F], vertexComponent: Uint32Array[V], triangles: Uint32Array[C], vertices: Uint32Array[C],
   *  invalidFaces }. */
  read() {
    const p = addon.meshComponentsGet(this.handle);
    const words = (ptr, n) => new Uint32Array(n ? this.device.readBuffer(this.device.view(ptr, 4 * n), 4 * n) : new ArrayBuffer(0));
    return { count: this.count, faceComponent: words(p[0], this.numFaces), vertexComponent: words(p[1], this.numVertices), triangles: words(p[2], this.count),
      vertices: words(p[3], this.count), invalidFaces: this.invalidFaces };
  }
  /** keep: one entry per component, truthy = kept.  Returns { vertices, faces }, the numbers kept (flags, scans; waits). */
  select(keep) {
    const r = addon.meshComponentsSelect(this.handle, Uint8Array.from(keep, (k) => (k ? 1 : 0)));
    return { vertices: r[0], faces: r[1] };
  }
  /** Writes the kept part for the last select: verticesOut f32[V'][3] gathered from vertices (both nullable together), facesOut u32[F'][3] renumbered,
   *  vertexMap u32[V'], faceMap u32[F'] (nullable).  WDGS_E_CAPACITY, with nothing written, when there is too little room.  Stream-ordered. */
  compact(vertices, verticesOut, facesOut, vertexMap, faceMap, capacityVertices, capacityFaces) {
    const room = (pairs) => Math.min(0xFFFFFFFF, ...pairs.filter(([b]) => b).map(([b, s]) => Math.floor(b.size / s)));
    const cv = capacityVertices === undefined || capacityVertices === null ? room([[verticesOut, 12], [vertexMap, 4]]) : capacityVertices;
    const cf = capacityFaces === undefined || capacityFaces === null ? room([[facesOut, 12], [faceMap, 4]]) : capacityFaces;
    for (const [b, s, n] of [[verticesOut, 12, cv], [vertexMap, 4, cv], [facesOut, 12, cf], [faceMap, 4, cf]]) {
      if (b && n * s > b.size) throw new Error('MeshComponents.compact: the capacity exceeds the buffers');
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshComponentsCompact(this.handle, ptr(vertices), ptr(verticesOut), ptr(facesOut), ptr(vertexMap), ptr(faceMap), cv, cf);
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshComponentsDestroy(this.handle); this.handle = null; }
}
/** The connected components of `mesh` ({ vertices, faces } as extractMesh returns them, or as HipBuffers): two vertices are connected when a face names
 *  both (shared vertices, not shared edges), components are numbered in ascending order of their lowest vertex, 0xFFFFFFFF marks a face that names a
 *  vertex >= V and a vertex that no face names.  A function of the mesh alone, bit for bit (include/webdgs.h states it). */
function meshComponents(device, mesh) {
  const v = asDevice(device, mesh.vertices, Float32Array, 3, 'meshComponents: vertices'), f = asDevice(device, mesh.faces, Uint32Array, 3, 'meshComponents: faces');
  const comp = new MeshComponents(device);
  try {
    comp.label(f.buf, f.rows, v.rows);
    return comp.read();
  } finally {
    comp.destroy();
    if (v.owned) v.buf.destroy();
    if (f.owned) f.buf.destroy();
  }
}
/** Which components to keep, from their sizes: ranked by (triangles descending, component number ascending), a component is kept when it is among the
 *  first keepLargest (null: all), has triangles >= minTriangles and triangles >= minFraction * largest (doubles).  options: { keepLargest, minTriangles,
 *  minFraction }.  Returns a Uint8Array[C] of 0 / 1.  Host side. */
function selectComponents(triangles, options) {
  const o = options || {}, C = triangles.length, keep = new Uint8Array(C);
  const all = o.keepLargest === undefined || o.keepLargest === null;
  if (!all && !(o.keepLargest >= 0)) throw new RangeError('selectComponents: keepLargest must be null or >= 0');
  const ranking = Array.from({ length: C }, (_, c) => c).sort((a, b) => (triangles[b] - triangles[a]) || (a - b));
  const largest = C ? triangles[ranking[0]] : 0, minTriangles = o.minTriangles || 0, minFraction = o.minFraction || 0;
  ranking.forEach((c, rank) => {
    if ((all || rank < o.keepLargest) && triangles[c] >= minTriangles && triangles[c] >= minFraction * largest) keep[c] = 1;
  });
  return keep;
}
/** `mesh` without the components selectComponents does not keep: { vertices, faces, vertexMap, faceMap, components } and colours / keys gathered through
 *  vertexMap when the input has them.  Kept faces stay in their order, kept vertices in ascending original index, faces are rewritten to the new indices;
 *  components holds the kept components' triangle counts.  Keeping everything still drops invalid faces and unreferenced vertices; a second call
 *  reproduces the first.  options: { keepLargest, minTriangles, minFraction, asBuffers }.  asBuffers: vertices, faces, vertexMap and faceMap stay on the
 *  device as HipBuffers (of at least one element's size) with numVertices and numFaces; colours and keys are not gathered; the caller destroys them. */
function removeSmallComponents(device, mesh, options) {
  const v = asDevice(device, mesh.vertices, Float32Array, 3, 'removeSmallComponents: vertices');
  const f = asDevice(device, mesh.faces, Uint32Array, 3, 'removeSmallComponents: faces');
  const comp = new MeshComponents(device);
  const outs = [];
  let out;
  try {
    comp.label(f.buf, f.rows, v.rows);
    const sizes = comp.read().triangles, keep = selectComponents(sizes, options);
    const kept = comp.select(keep);
    for (const n of [12 * kept.vertices, 12 * kept.faces, 4 * kept.vertices, 4 * kept.faces]) outs.push(device.createBuffer({ size: Math.max(n, 4), label: 'compacted mesh' }));
    comp.compact(v.buf, outs[0], outs[1], outs[2], outs[3], kept.vertices, kept.faces);
    if (options && options.asBuffers) {
      device.synchronize();   // (an uploaded mesh is released below)
      const result = { vertices: outs[0], faces: outs[1], vertexMap: outs[2], faceMap: outs[3], numVertices: kept.vertices, numFaces: kept.faces,
        components: sizes.filter((_, c) => keep[c]) };
      outs.length = 0;
      return result;
    }
    const bytes = (b, n) => (n ? device.readBuffer(b, n) : new ArrayBuffer(0));
    out = { vertices: new Float32Array(bytes(outs[0], 12 * kept.vertices)), faces: new Uint32Array(bytes(outs[1], 12 * kept.faces)),
      vertexMap: new Uint32Array(bytes(outs[2], 4 * kept.vertices)), faceMap: new Uint32Array(bytes(outs[3], 4 * kept.faces)),
      components: sizes.filter((_, c) => keep[c]) };
  } finally {
    comp.destroy();
    if (v.owned) v.buf.destroy();
    if (f.owned) f.buf.destroy();
    outs.forEach((b) => b.destroy());
  }
  if (mesh.colours !== undefined) {
    out.colours = mesh.colours ? new Uint8Array(3 * out.vertexMap.length) : null;
    if (out.colours) out.vertexMap.forEach((old, i) => { for (let a = 0; a < 3; a++) out.colours[3 * i + a] = mesh.colours[3 * old + a]; });
  }
  if (mesh.keys !== undefined) out.keys = mesh.keys ? BigUint64Array.from(out.vertexMap, (old) => mesh.keys[old]) : null;
  return out;
}
// ---------------------------------------------------------------- per-face visibility and removal of unseen faces (include/webdgs.h, DESIGN.md section 21)
const VISIBILITY_STATS = ['views', 'foreignPixels', 'countedPixels', 'agreeingPixels'];
const invalidArgument = (message) => { const e = new Error(message); e.code = 'WDGS_E'; return e; };
/** rint(fraction 65536) for a fraction in [0, 1], ties to even: what wdgs_face_visibility_flags compares with. */
function fractionQ16(fraction, what) {
  const x = fraction === undefined || fraction === null ? 0 : Number(fraction);
  if (!(x >= 0 && x <= 1)) throw invalidArgument(`${what}: minAgreeingFraction ${fraction} is not in [0, 1]`);
  const y = x * 65536, f = Math.floor(y), d = y - f;
  return d > 0.5 || (d === 0.5 && f % 2 === 1) ? f + 1 : f;
}
/** [minPixels, minViews, minAgreeing, q16] of a rule { minPixels = 1, minViews = 1, minAgreeing = 0, minAgreeingFraction = 0 }. */
function faceRule(rule, what) {
  const o = rule || {}, pick = (v, d) => (v === undefined || v === null ? d : v);
  const counts = [pick(o.minPixels, 1), pick(o.minViews, 1), pick(o.minAgreeing, 0)];
  if (!counts.every((x) => Number.isInteger(x) && x >= 0 && x < 2 ** 32)) throw invalidArgument(`${what}: minPixels, minViews, minAgreeing ${counts} must fit 32 unsigned bits`);
  return counts.concat([fractionQ16(o.minAgreeingFraction, what)]);
}
/** Per-face counters over views (wdgs_face_visibility): reset sizes them for a mesh, accumulate adds one view -- the face image MeshRasterizer.encode wrote
 *  and, optionally, the mesh's and the model's depth images -- read / buffer hand out u32[F][3] = { pixels, agreeing, views }, flags applies the rule on the
 *  device and stats reads the totals.  Integer sums: every byte is a function of the inputs.  faceVisibility is the one-call form without a model. */
class FaceVisibility {
  constructor(device) { this.device = device; this.destroyed = false; this.numFaces = 0; this.handle = addon.faceVisibilityCreate(device.handle); }
  /** Sizes and zeroes the counters for numFaces faces; the accumulated views start at 0.  A call that grows the arrays waits once. */
  reset(numFaces) { addon.faceVisibilityReset(this.handle, numFaces); this.numFaces = numFaces; }
  /** One view of width x height: faceImage u32, and both or neither of options.meshDepth and options.modelDepth f32 (options.modelWeightSum beside them,
   *  optional; options.minWeightSum = 0, options.threshold = 0.05).  Stream-ordered, recordable.  WDGS_E_CAPACITY, with nothing written, when one more view
   *  of this size could carry a pixel count past 32 bits. */
  accumulate(faceImage, width, height, options) {
    const o = options || {};
    if (width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE) {
      for (const b of [faceImage, o.meshDepth, o.modelDepth, o.modelWeightSum]) if (b && b.size < 4 * width * height) throw new Error(`FaceVisibility.accumulate: an image is too small for ${width}x${height}`);
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.faceVisibilityAccumulate(this.handle, ptr(faceImage), ptr(o.meshDepth), ptr(o.modelDepth), ptr(o.modelWeightSum), Math.fround(o.minWeightSum || 0),
      Math.fround(o.threshold === undefined || o.threshold === null ? 0.05 : o.threshold), width, height);
  }
  /** The counters u32[F][3] on the device as of this call (one launch writes them; null for no faces), valid until the next buffer, read, reset or destroy. */
  buffer() {
    const p = addon.faceVisibilityGet(this.handle);
    return this.numFaces ? this.device.view(p, 12 * this.numFaces) : null;
  }
  /** The counters as a Uint32Array[3 F]: pixels, agreeing, views per face (waits). */
  read() { const b = this.buffer(); return new Uint32Array(b ? this.device.readBuffer(b, 12 * this.numFaces) : new ArrayBuffer(0)); }
  /** keep u8[F] on the device from the current counters, by selectFaces' rule.  Stream-ordered, recordable. */
  flags(keep, rule) { encodeFaceVisibilityFlags(this.device, this.buffer(), this.numFaces, keep, rule); }
  /** { views, foreignPixels, countedPixels, agreeingPixels } since the reset (waits). */
  stats() { const r = addon.faceVisibilityStats(this.handle), out = {}; VISIBILITY_STATS.forEach((k, i) => { out[k] = r[i]; }); return out; }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.faceVisibilityDestroy(this.handle); this.handle = null; }
}
/** wdgs_face_visibility_flags: keep u8[numFaces] from counters u32[numFaces][3], both on the device.  Stream-ordered, recordable. */
function encodeFaceVisibilityFlags(device, counters, numFaces, keep, rule) {
  const r = faceRule(rule, 'faceVisibilityFlags');
  if (numFaces < 2 ** 31 && ((counters && counters.size < 12 * numFaces) || (keep && keep.size < numFaces))) throw new Error('faceVisibilityFlags: buffers too small for the faces');
  addon.faceVisibilityFlags(device.handle, counters ? counters.ptr : null, numFaces, r[0], r[1], r[2], r[3], keep ? keep.ptr : null);
}
/** Which faces to keep, a Uint8Array[F] of 0 / 1, from counters Uint32Array[3 F] = { pixels, agreeing, views } per face: pixels >= minPixels, views >= minViews,
 *  agreeing >= minAgreeing and agreeing 65536 >= rint(minAgreeingFraction 65536) pixels in 64-bit integers.  The host restatement of FaceVisibility.flags. */
function selectFaces(counters, rule) {
  const r = faceRule(rule, 'selectFaces'), F = Math.floor(counters.length / 3), keep = new Uint8Array(F), q16 = BigInt(r[3]);
  for (let f = 0; f < F; f++) {
    const pixels = counters[3 * f], agreeing = counters[3 * f + 1], views = counters[3 * f + 2];
    keep[f] = pixels >= r[0] && views >= r[1] && agreeing >= r[2] && BigInt(agreeing) * 65536n >= q16 * BigInt(pixels) ? 1 : 0;
  }
  return keep;
}
/** MeshComponents' compaction for an arbitrary face mask (wdgs_mesh_face_filter): select takes the faces and a u8 flag per face on the device, compact writes
 *  the kept part.  filterFaces is the one-call form. */
class MeshFaceFilter {
  constructor(device) { this.device = device; this.destroyed = false; this.handle = addon.meshFaceFilterCreate(device.handle); }
  /** { vertices, faces, invalidFaces }: the numbers kept of faces u32[numFaces][3] over numVertices vertices under keep u8[numFaces], and the faces that name
   *  no vertex (flags, scans; waits). */
  select(faces, numFaces, numVertices, keep) {
    if (numFaces < 2 ** 31 && ((faces && faces.size < 12 * numFaces) || (keep && keep.size < numFaces))) throw new Error('MeshFaceFilter.select: buffers too small for the faces');
    const r = addon.meshFaceFilterSelect(this.handle, faces ? faces.ptr : null, numFaces, numVertices, keep ? keep.ptr : null);
    return { vertices: r[0], faces: r[1], invalidFaces: r[2] };
  }
  /** MeshComponents.compact's arguments and rules for the last select.  Stream-ordered, recordable. */
  compact(vertices, verticesOut, facesOut, vertexMap, faceMap, capacityVertices, capacityFaces) {
    const room = (pairs) => Math.min(0xFFFFFFFF, ...pairs.filter(([b]) => b).map(([b, s]) => Math.floor(b.size / s)));
    const cv = capacityVertices === undefined || capacityVertices === null ? room([[verticesOut, 12], [vertexMap, 4]]) : capacityVertices;
    const cf = capacityFaces === undefined || capacityFaces === null ? room([[facesOut, 12], [faceMap, 4]]) : capacityFaces;
    for (const [b, s, n] of [[verticesOut, 12, cv], [vertexMap, 4, cv], [facesOut, 12, cf], [faceMap, 4, cf]]) {
      if (b && n * s > b.size) throw new Error('MeshFaceFilter.compact: the capacity exceeds the buffers');
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshFaceFilterCompact(this.handle, ptr(vertices), ptr(verticesOut), ptr(facesOut), ptr(vertexMap), ptr(faceMap), cv, cf);
  }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshFaceFilterDestroy(this.handle); this.handle = null; }
}
/** `mesh` without the faces whose keep flag (an array of F truthy / falsy values, or a u8[F] HipBuffer) is zero, and without the vertices no kept face names:
 *  { vertices, faces, vertexMap, faceMap, invalidFaces } and colours / keys gathered through vertexMap when the input has them -- removeSmallComponents' shape
 *  and rules.  `mesh`: typed arrays, or an object of HipBuffers as meshOnDevice takes (left as it is).  options.asBuffers: the four arrays stay on the device
 *  as HipBuffers (of at least one element's size) with numVertices and numFaces; colours and keys are not gathered; the caller destroys them. */
function filterFaces(device, mesh, keep, options) {
  const src = meshOnDevice(device, mesh, 'filterFaces');
  const outs = [];
  let kbuf = keep, ownKeep = false, filt = null, out;
  try {
    if (!(keep instanceof HipBuffer)) {
      if (keep.length !== src.F) throw new Error(`filterFaces: ${keep.length} flags for ${src.F} faces`);
      kbuf = device.createBuffer({ size: Math.max(src.F, 8), label: 'filterFaces: flags' }); ownKeep = true;
      if (src.F) device.queue.writeBuffer(kbuf, 0, Uint8Array.from(keep, (k) => (k ? 1 : 0)));
    }
    filt = new MeshFaceFilter(device);
    const kept = filt.select(src.faces, src.F, src.V, kbuf);
    for (const n of [12 * kept.vertices, 12 * kept.faces, 4 * kept.vertices, 4 * kept.faces]) outs.push(device.createBuffer({ size: Math.max(n, 4), label: 'filtered mesh' }));
    filt.compact(src.vertices, outs[0], outs[1], outs[2], outs[3], kept.vertices, kept.faces);
    if (options && options.asBuffers) {
      device.synchronize();   // (an uploaded mesh is released below)
      const result = { vertices: outs[0], faces: outs[1], vertexMap: outs[2], faceMap: outs[3], numVertices: kept.vertices, numFaces: kept.faces, invalidFaces: kept.invalidFaces };
      outs.length = 0;
      return result;
    }
    const bytes = (b, n) => (n ? device.readBuffer(b, n) : new ArrayBuffer(0));
    out = { vertices: new Float32Array(bytes(outs[0], 12 * kept.vertices)), faces: new Uint32Array(bytes(outs[1], 12 * kept.faces)),
      vertexMap: new Uint32Array(bytes(outs[2], 4 * kept.vertices)), faceMap: new Uint32Array(bytes(outs[3], 4 * kept.faces)), invalidFaces: kept.invalidFaces };
  } finally {
    if (filt) filt.destroy();
    if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
    if (ownKeep) kbuf.destroy();
    outs.forEach((b) => b.destroy());
  }
  gatherVertexAttributes(mesh, out);
  return out;
}
/** colours (three bytes per vertex) and keys of a typed-array mesh, gathered through out.vertexMap into out. */
function gatherVertexAttributes(mesh, out) {
  if (mesh.colours !== undefined && !(mesh.colours instanceof HipBuffer)) {
    out.colours = mesh.colours ? new Uint8Array(3 * out.vertexMap.length) : null;
    if (out.colours) out.vertexMap.forEach((old, i) => { for (let a = 0; a < 3; a++) out.colours[3 * i + a] = mesh.colours[3 * old + a]; });
  }
  if (mesh.keys !== undefined && !(mesh.keys instanceof HipBuffer)) out.keys = mesh.keys ? BigUint64Array.from(out.vertexMap, (old) => mesh.keys[old]) : null;
}
/** Which faces of `mesh` the `cameras` (68-float blocks: Float32Arrays or HipBuffers) see, without a model: every camera's face image is rasterized at
 *  width x height and accumulated.  { counters: Uint32Array[3 F], stats }; agreeing equals pixels here.  options: { near = MESH_RASTER_NEAR, cull = 'none' }.
 *  selectFaces and filterFaces take it from there. */
function faceVisibility(device, mesh, cameras, width, height, options) {
  const o = options || {}, src = meshOnDevice(device, mesh, 'faceVisibility');
  let rasterizer = null, visibility = null, image = null;
  try {
    rasterizer = new MeshRasterizer(device); visibility = new FaceVisibility(device);
    visibility.reset(src.F);
    const npix = width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE ? width * height : 0;
    image = device.createBuffer({ size: Math.max(4 * npix, 16), label: 'mesh face image' });
    for (const camera of cameras) {
      let cam = camera;
      if (!(camera instanceof HipBuffer)) {
        if (camera.length !== 68) throw new Error(`faceVisibility: the camera block has 68 floats, got ${camera.length}`);
        cam = device.createBuffer({ size: 272 });
        device.queue.writeBuffer(cam, 0, camera instanceof Float32Array ? camera : Float32Array.from(camera));
      }
      try {
        rasterizer.encode(src.vertices, src.V, src.faces, src.F, null, cam, width, height, { near: o.near, cull: o.cull, face: image });
        visibility.accumulate(image, width, height);
      } finally {
        if (cam !== camera) { device.synchronize(); cam.destroy(); }
      }
    }
    return { counters: visibility.read(), stats: visibility.stats() };
  } finally {
    for (const x of [visibility, rasterizer, image]) if (x) x.destroy();
    if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
  }
}
// ---------------------------------------------------------------- vertex colours baked from photographs (include/webdgs.h, DESIGN.md section 22)
const BAKE_STATS = ['usable', 'inImage', 'visible', 'accumulated', 'viewportMismatch', 'bakedVertices'];
/** Per-vertex colour sums over views (wdgs_mesh_colour_baker): reset sizes them for a mesh, accumulate adds one view -- a photograph, its camera block and,
 *  optionally, the vertex normals (the weights) and the depth image MeshRasterizer.encode wrote for this mesh and camera (the occlusion test) -- resolve turns
 *  the sums into rgba8 vertex colours, read hands out the sums and stats the totals.  Integer sums: the state does not depend on the order of the views and
 *  every byte is a function of the inputs.  bakeVertexColours is the one-call form. */
class MeshColourBaker {
  constructor(device) { this.device = device; this.destroyed = false; this.numVertices = 0; this.handle = addon.meshColourBakerCreate(device.handle); }
  /** Sizes and zeroes the state for numVertices vertices.  A call that grows the arrays waits once; it cannot be recorded. */
  reset(numVertices) { addon.meshColourBakerReset(this.handle, numVertices); this.numVertices = numVertices; }
  /** One view of width x height: vertices f32[numVertices][3], the 68-float camera block, image rgba8; options: { normals, meshDepth (HipBuffers or null),
   *  near = MESH_RASTER_NEAR, depthTolerance = 0.05, minCos = 0.1 }.  Stream-ordered, recordable. */
  accumulate(vertices, numVertices, camera, image, width, height, options) {
    const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v);
    if (numVertices < 2 ** 31 && [vertices, o.normals].some((b) => b && b.size < 12 * numVertices)) throw new Error('MeshColourBaker.accumulate: buffers too small for the vertices');
    if (camera && camera.size < 272) throw new Error('MeshColourBaker.accumulate: the camera block has 68 floats');
    if (width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE) {
      for (const b of [image, o.meshDepth]) if (b && b.size < 4 * width * height) throw new Error(`MeshColourBaker.accumulate: an image is too small for ${width}x${height}`);
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshColourBakerAccumulate(this.handle, ptr(vertices), ptr(o.normals), numVertices, ptr(camera), ptr(image), ptr(o.meshDepth), width, height,
      Math.fround(pick(o.near, MESH_RASTER_NEAR)), Math.fround(pick(o.depthTolerance, 0.05)), Math.fround(pick(o.minCos, 0.1)));
  }
  /** coloursOut rgba8[numVertices] from the current sums; options: { fallback (may be coloursOut itself), bakedOut u8[numVertices], minViews = 1,
   *  minWeight = 1 (a number or a BigInt) }.  Stream-ordered, recordable. */
  resolve(coloursOut, numVertices, options) {
    const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v), minViews = pick(o.minViews, 1), minWeight = pick(o.minWeight, 1);
    if (!(Number.isInteger(minViews) && minViews >= 0 && minViews < 2 ** 32) || !(typeof minWeight === 'bigint' ? minWeight >= 0n && minWeight < 2n ** 64n : Number.isInteger(minWeight) && minWeight >= 0)) {
      const e = new Error(`MeshColourBaker.resolve: bad thresholds ${minViews}, ${minWeight}`); e.code = 'WDGS_E'; throw e;
    }
    if (numVertices < 2 ** 31 && ([coloursOut, o.fallback].some((b) => b && b.size < 4 * numVertices) || (o.bakedOut && o.bakedOut.size < numVertices))) throw new Error('MeshColourBaker.resolve: buffers too small for the vertices');
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshColourBakerResolve(this.handle, ptr(coloursOut), ptr(o.fallback), ptr(o.bakedOut), numVertices, minViews, minWeight);
  }
  /** { sums: BigUint64Array[4 V] (R, G, B, Wt per vertex), views: Uint32Array[V] } (waits). */
  read() { const r = addon.meshColourBakerRead(this.handle, this.numVertices); return { sums: new BigUint64Array(r[0]), views: new Uint32Array(r[1]) }; }
  /** { usable, inImage, visible, accumulated, viewportMismatch, bakedVertices }: the vertices that passed each step summed over the views since the reset, the
   *  calls whose camera block was of another image size, and the baked vertices of the last resolve (waits). */
  stats() { const r = addon.meshColourBakerStats(this.handle), out = {}; BAKE_STATS.forEach((k, i) => { out[k] = r[i]; }); return out; }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshColourBakerDestroy(this.handle); this.handle = null; }
}
/** bakeVertexColours for views that are on the device already: `views` is an array of { camera, image, width, height } with HipBuffers, which may differ in
 *  size (Evaluator.bakeMeshColours hands in the trainer's own cameras and photographs).  options: bakeVertexColours'. */
function bakeMeshFromViews(device, mesh, views, options, what) {
  const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v), name = what || 'bakeVertexColours';
  const occlusion = pick(o.occlusion, true), src = meshOnDevice(device, mesh, name), V = src.V, owned = src.own ? [src.vertices, src.faces] : [];
  const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); owned.push(b); return b; };
  let baker = null, rasterizer = null, depth = null, out = {};
  try {
    let fallback = null, normals = null;
    const c = mesh.colours;
    if (c instanceof HipBuffer) fallback = c;
    else if (c) {
      let rgba = c;
      if (c.length === 3 * V) {
        rgba = new Uint8Array(4 * V).fill(255);
        for (let v = 0; v < V; v++) for (let a = 0; a < 3; a++) rgba[4 * v + a] = c[3 * v + a];
      } else if (c.length !== 4 * V) throw new Error(`${name}: ${c.length} colour bytes for ${V} vertices`);
      fallback = upload(rgba instanceof Uint8Array ? rgba : Uint8Array.from(rgba));
    }
    if (pick(o.normals, true)) {
      const n = mesh.normals;
      if (n instanceof HipBuffer) normals = n;
      else if (n) {
        if (n.length !== 3 * V) throw new Error(`${name}: ${n.length} normal components for ${V} vertices`);
        normals = upload(n instanceof Float32Array ? n : Float32Array.from(n));
      } else { normals = smoothAndNormals(device, src.vertices, src.faces, V, src.F, null, true).normals; owned.push(normals); }
    }
    const legal = views.filter((w) => w.width >= 1 && w.width <= MESH_RASTER_MAX_SIZE && w.height >= 1 && w.height <= MESH_RASTER_MAX_SIZE);
    baker = new MeshColourBaker(device);
    baker.reset(V);
    if (occlusion && legal.length) {   // (the rasterizer is grown once, to the largest view, in front of the loop)
      const big = legal.reduce((a, w) => (w.width * w.height > a.width * a.height ? w : a), legal[0]);
      depth = device.createBuffer({ size: Math.max(4 * big.width * big.height, 16), label: 'mesh depth' });
      rasterizer = new MeshRasterizer(device);
      rasterizer.encode(src.vertices, V, src.faces, src.F, null, big.camera, big.width, big.height, { near: o.near, depth });
    }
    for (const w of views) {
      if (rasterizer && legal.includes(w)) rasterizer.encode(src.vertices, V, src.faces, src.F, null, w.camera, w.width, w.height, { near: o.near, depth });
      baker.accumulate(src.vertices, V, w.camera, w.image, w.width, w.height, { normals, meshDepth: occlusion ? depth : null, near: o.near, depthTolerance: o.depthTolerance, minCos: o.minCos });
    }
    out = { colours: device.createBuffer({ size: Math.max(4 * V, 8), label: 'baked colours' }), baked: device.createBuffer({ size: Math.max(V, 8), label: 'baked mask' }) };
    baker.resolve(out.colours, V, { fallback, bakedOut: out.baked, minViews: o.minViews, minWeight: o.minWeight });
    const stats = baker.stats();   // (waits: the objects released below are idle)
    if (o.asBuffers) { const result = Object.assign({}, mesh, out, { stats }); out = {}; return result; }
    const rgba = new Uint8Array(V ? device.readBuffer(out.colours, 4 * V) : new ArrayBuffer(0)), colours = new Uint8Array(3 * V);
    for (let v = 0; v < V; v++) for (let a = 0; a < 3; a++) colours[3 * v + a] = rgba[4 * v + a];
    return Object.assign({}, mesh, { colours, baked: new Uint8Array(V ? device.readBuffer(out.baked, V) : new ArrayBuffer(0)), stats });
  } finally {
    for (const x of [baker, rasterizer, depth]) if (x) x.destroy();
    destroyBuffers(out);
    device.synchronize();
    owned.forEach((b) => b.destroy());
  }
}
/** `mesh` with its vertex colours taken from photographs, without a model: per camera (68-float blocks: Float32Arrays or HipBuffers) and its image (rgba8
 *  Uint8Array[height * width * 4], or a HipBuffer) the mesh's depth image is rasterized (options.occlusion) and every vertex that projects into the photograph,
 *  is not hidden (all four depth texels round it within depthTolerance of its own depth) and faces the camera adds the bilinear sample there, weighted by the
 *  cosine between its normal and the direction to the camera.  A vertex at least minViews views coloured, with a weight sum of at least minWeight (256 per
 *  view that looks straight at it), gets the weighted mean; any other keeps the mesh's own colour (zeros without colours).  options: { normals = true (the
 *  mesh's, or vertexNormals' when it carries none; false: every view weighs the same), depthTolerance = 0.05, minCos = 0.1 (a caller's knob, not a tuned
 *  number), minViews = 1, minWeight = 1, near = MESH_RASTER_NEAR, occlusion = true, asBuffers }.  Returns the mesh's object with colours: Uint8Array[3 V]
 *  replaced and baked: Uint8Array[V] and stats added; asBuffers: colours rgba8[V] and baked u8[V] stay on the device.  Same results as the Python host's. */
function bakeVertexColours(device, mesh, cameras, images, width, height, options) {
  if (cameras.length !== images.length) throw new Error(`bakeVertexColours: ${cameras.length} cameras for ${images.length} images`);
  const owned = [];
  const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); owned.push(b); return b; };
  try {
    const views = cameras.map((camera, k) => {
      let cam = camera, image = images[k];
      if (!(camera instanceof HipBuffer)) {
        if (camera.length !== 68) throw new Error(`bakeVertexColours: the camera block has 68 floats, got ${camera.length}`);
        cam = upload(camera instanceof Float32Array ? camera : Float32Array.from(camera));
      }
      if (!(image instanceof HipBuffer)) {
        if (image.length !== 4 * width * height) throw new Error(`bakeVertexColours: an image of ${image.length} bytes for ${width}x${height} rgba8`);
        image = upload(image instanceof Uint8Array ? image : Uint8Array.from(image));
      }
      return { camera: cam, image, width, height };
    });
    return bakeMeshFromViews(device, mesh, views, options);
  } finally {
    device.synchronize();
    owned.forEach((b) => b.destroy());
  }
}
// ---------------------------------------------------------------- a texture atlas baked from photographs (include/webdgs.h, DESIGN.md section 23)
const TEXTURE_STATS = ['invalidFaces', 'facingAwayFaces', 'offImageFaces', 'usable', 'inImage', 'visible', 'accumulated', 'viewportMismatch', 'bakedTexels',
  'filledTexels', 'fallbackTexels'];
const MESH_TEXTURE_MAX_SIZE = 16384;
/** The atlas of numFaces faces in square cells of `cell` texels (4, 8, 16 or 32; default 8), two faces per cell: { width, height, cellsPerRow,
 *  uv: Float32Array[F * 3 * 2] } with the per-corner texture coordinates in the OBJ convention -- u = (x + 0.5) / width, v = 1 - (y + 0.5) / height for the
 *  atlas texel (x, y) a corner sits on, computed in doubles and rounded once.  Arithmetic alone; the same bytes as the Python host's. */
function textureLayout(numFaces, cell) {
  const F = numFaces, c = cell === undefined || cell === null ? 8 : cell;
  if (!(Number.isInteger(F) && F >= 0 && F < 2 ** 31)) throw new Error(`textureLayout: ${numFaces} faces (0 to 2^31 - 1)`);
  if (![4, 8, 16, 32].includes(c)) throw new Error(`textureLayout: a cell of ${cell} texels (4, 8, 16 or 32)`);
  const cells = Math.floor((F + 1) / 2);
  let perRow = Math.floor(Math.sqrt(cells));
  while (perRow * perRow < cells) perRow++;
  while (perRow > 0 && (perRow - 1) * (perRow - 1) >= cells) perRow--;
  const rows = perRow ? Math.ceil(cells / perRow) : 0, width = perRow * c, height = rows * c, m = c - 3;
  if (width > MESH_TEXTURE_MAX_SIZE) throw new Error(`textureLayout: ${F} faces in cells of ${c} texels need an atlas ${width} texels wide (at most ${MESH_TEXTURE_MAX_SIZE})`);
  const uv = new Float32Array(6 * F), corner = [[0, 0], [m, 0], [0, m]];
  for (let f = 0; f < F; f++) {
    const k = Math.floor(f / 2), odd = f % 2;
    for (let n = 0; n < 3; n++) {
      const i = odd ? c - 1 - corner[n][0] : corner[n][0], j = odd ? c - 1 - corner[n][1] : corner[n][1];
      uv[6 * f + 2 * n] = ((k % perRow) * c + i + 0.5) / width;
      uv[6 * f + 2 * n + 1] = 1.0 - (Math.floor(k / perRow) * c + j + 0.5) / height;
    }
  }
  return { width, height, cellsPerRow: perRow, uv };
}
/** Per-texel colour sums of a mesh's texture atlas over views (wdgs_mesh_texture_baker): reset lays the atlas out for a face count and a cell size and zeroes
 *  the sums, accumulate adds one view, resolve turns the sums into an rgba8 texture, read hands out the sums and stats the totals.  Integer sums: the state does
 *  not depend on the order of the views and every byte is a function of the inputs.  bakeTexture is the one-call form. */
class MeshTextureBaker {
  constructor(device) {
    this.device = device; this.destroyed = false; this.numFaces = this.cell = this.width = this.height = this.cellsPerRow = 0;
    this.handle = addon.meshTextureBakerCreate(device.handle);
  }
  /** Lays the atlas out and zeroes the state; returns { width, height, cellsPerRow }.  A call that grows the array waits once; it cannot be recorded.
   *  accumulates: where the count of views starts, for the test of the refusal of the 65536th. */
  reset(numFaces, cell, accumulates) {
    const c = cell === undefined || cell === null ? 8 : cell, r = addon.meshTextureBakerReset(this.handle, numFaces, c, accumulates || 0);
    this.numFaces = numFaces; this.cell = c; [this.width, this.height, this.cellsPerRow] = r;
    return { width: r[0], height: r[1], cellsPerRow: r[2] };
  }
  /** One view of width x height; options: { meshDepth (a HipBuffer or null), near = MESH_RASTER_NEAR, depthTolerance = 0.05, minCos = 0.1, twoSided = false }.
   *  Stream-ordered, recordable. */
  accumulate(vertices, numVertices, faces, numFaces, camera, image, width, height, options) {
    const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v);
    if ((numVertices < 2 ** 31 && vertices && vertices.size < 12 * numVertices) || (numFaces < 2 ** 31 && faces && faces.size < 12 * numFaces)) throw new Error('MeshTextureBaker.accumulate: buffers too small for the mesh');
    if (camera && camera.size < 272) throw new Error('MeshTextureBaker.accumulate: the camera block has 68 floats');
    if (width >= 1 && width <= MESH_RASTER_MAX_SIZE && height >= 1 && height <= MESH_RASTER_MAX_SIZE) {
      for (const b of [image, o.meshDepth]) if (b && b.size < 4 * width * height) throw new Error(`MeshTextureBaker.accumulate: an image is too small for ${width}x${height}`);
    }
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshTextureBakerAccumulate(this.handle, ptr(vertices), numVertices, ptr(faces), numFaces, ptr(camera), ptr(image), ptr(o.meshDepth), width, height,
      Math.fround(pick(o.near, MESH_RASTER_NEAR)), Math.fround(pick(o.depthTolerance, 0.05)), Math.fround(pick(o.minCos, 0.1)), o.twoSided ? 1 : 0);
  }
  /** textureOut rgba8[height][width] from the current sums; options: { colours rgba8[numVertices], stateOut u8[height][width], minWeight = 1, fill = true }.
   *  Stream-ordered, recordable. */
  resolve(faces, numFaces, numVertices, textureOut, options) {
    const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v), minWeight = pick(o.minWeight, 1), n = this.width * this.height;
    if (!(Number.isInteger(minWeight) && minWeight >= 0 && minWeight < 2 ** 32)) { const e = new Error(`MeshTextureBaker.resolve: bad threshold ${minWeight}`); e.code = 'WDGS_E'; throw e; }
    if ((textureOut && textureOut.size < 4 * n) || (o.stateOut && o.stateOut.size < n)) throw new Error(`MeshTextureBaker.resolve: an output is too small for ${this.width}x${this.height}`);
    if ((numFaces < 2 ** 31 && faces && faces.size < 12 * numFaces) || (numVertices < 2 ** 31 && o.colours && o.colours.size < 4 * numVertices)) throw new Error('MeshTextureBaker.resolve: buffers too small for the mesh');
    const ptr = (b) => (b ? b.ptr : null);
    addon.meshTextureBakerResolve(this.handle, ptr(faces), numFaces, numVertices, ptr(o.colours), ptr(textureOut), ptr(o.stateOut), minWeight, pick(o.fill, true) ? 1 : 0);
  }
  /** Uint32Array[4 * cells * cell * cell]: R, G, B, Wsum per texel, cell-major (waits). */
  read() { return new Uint32Array(addon.meshTextureBakerRead(this.handle, Math.floor((this.numFaces + 1) / 2) * this.cell * this.cell)); }
  /** The eleven totals by name (waits). */
  stats() { const r = addon.meshTextureBakerStats(this.handle), out = {}; TEXTURE_STATS.forEach((k, i) => { out[k] = r[i]; }); return out; }
  destroy() { if (this.destroyed) return; this.destroyed = true; addon.meshTextureBakerDestroy(this.handle); this.handle = null; }
}
/** bakeTexture for views that are on the device already: `views` is an array of { camera, image, width, height } with HipBuffers, which may differ in size.
 *  options: bakeTexture's. */
function bakeTextureFromViews(device, mesh, views, options, what) {
  const o = options || {}, pick = (v, d) => (v === undefined || v === null ? d : v), name = what || 'bakeTexture';
  const occlusion = pick(o.occlusion, true), cell = pick(o.cell, 8), src = meshOnDevice(device, mesh, name), V = src.V, F = src.F, owned = src.own ? [src.vertices, src.faces] : [];
  const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); owned.push(b); return b; };
  let baker = null, rasterizer = null, depth = null, out = {};
  try {
    let colours = null;
    const c = mesh.colours;
    if (c instanceof HipBuffer) colours = c;
    else if (c) {
      let rgba = c;
      if (c.length === 3 * V) {
        rgba = new Uint8Array(4 * V).fill(255);
        for (let v = 0; v < V; v++) for (let a = 0; a < 3; a++) rgba[4 * v + a] = c[3 * v + a];
      } else if (c.length !== 4 * V) throw new Error(`${name}: ${c.length} colour bytes for ${V} vertices`);
      colours = upload(rgba instanceof Uint8Array ? rgba : Uint8Array.from(rgba));
    }
    const layout = textureLayout(F, cell), n = layout.width * layout.height;
    const legal = views.filter((w) => w.width >= 1 && w.width <= MESH_RASTER_MAX_SIZE && w.height >= 1 && w.height <= MESH_RASTER_MAX_SIZE);
    baker = new MeshTextureBaker(device);
    baker.reset(F, cell);
    if (occlusion && legal.length) {   // (the rasterizer is grown once, to the largest view, in front of the loop)
      const big = legal.reduce((a, w) => (w.width * w.height > a.width * a.height ? w : a), legal[0]);
      depth = device.createBuffer({ size: Math.max(4 * big.width * big.height, 16), label: 'mesh depth' });
      rasterizer = new MeshRasterizer(device);
      rasterizer.encode(src.vertices, V, src.faces, F, null, big.camera, big.width, big.height, { near: o.near, depth });
    }
    for (const w of views) {
      if (rasterizer && legal.includes(w)) rasterizer.encode(src.vertices, V, src.faces, F, null, w.camera, w.width, w.height, { near: o.near, depth });
      baker.accumulate(src.vertices, V, src.faces, F, w.camera, w.image, w.width, w.height, { meshDepth: occlusion ? depth : null, near: o.near, depthTolerance: o.depthTolerance,
        minCos: o.minCos, twoSided: o.twoSided });
    }
    out = { texture: device.createBuffer({ size: Math.max(4 * n, 8), label: 'baked texture' }), texelState: device.createBuffer({ size: Math.max(n, 8), label: 'texel state' }) };
    baker.resolve(src.faces, F, V, out.texture, { colours, stateOut: out.texelState, minWeight: o.minWeight, fill: o.fill });
    const textureStats = baker.stats();   // (waits: the objects released below are idle)
    const extra = { uv: layout.uv, textureWidth: layout.width, textureHeight: layout.height, textureCell: cell, textureStats };
    if (o.asBuffers) { const result = Object.assign({}, mesh, out, extra); out = {}; return result; }
    return Object.assign({}, mesh, { texture: new Uint8Array(n ? device.readBuffer(out.texture, 4 * n) : new ArrayBuffer(0)),
      texelState: new Uint8Array(n ? device.readBuffer(out.texelState, n) : new ArrayBuffer(0)) }, extra);
  } finally {
    for (const x of [baker, rasterizer, depth]) if (x) x.destroy();
    destroyBuffers(out);
    device.synchronize();
    owned.forEach((b) => b.destroy());
  }
}
/** `mesh` with a texture atlas taken from photographs, without a model (the Python host's ops.bakeTexture).  options: { cell = 8, depthTolerance = 0.05,
 *  minCos = 0.1, minWeight = 1, near = MESH_RASTER_NEAR, occlusion = true, twoSided = false, fill = true, asBuffers }.  Returns the mesh's object with
 *  texture: Uint8Array[Ht * Wt * 4] (row 0 at the top), uv: Float32Array[F * 6], texelState: Uint8Array[Ht * Wt] (1 baked, 2 filled, 0 otherwise),
 *  textureWidth, textureHeight, textureCell and textureStats added; asBuffers: texture and texelState stay on the device.  Same results as the Python host's. */
function bakeTexture(device, mesh, cameras, images, width, height, options) {
  if (cameras.length !== images.length) throw new Error(`bakeTexture: ${cameras.length} cameras for ${images.length} images`);
  const owned = [];
  const upload = (a) => { const b = device.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) device.queue.writeBuffer(b, 0, a); owned.push(b); return b; };
  try {
    const views = cameras.map((camera, k) => {
      let cam = camera, image = images[k];
      if (!(camera instanceof HipBuffer)) {
        if (camera.length !== 68) throw new Error(`bakeTexture: the camera block has 68 floats, got ${camera.length}`);
        cam = upload(camera instanceof Float32Array ? camera : Float32Array.from(camera));
      }
      if (!(image instanceof HipBuffer)) {
        if (image.length !== 4 * width * height) throw new Error(`bakeTexture: an image of ${image.length} bytes for ${width}x${height} rgba8`);
        image = upload(image instanceof Uint8Array ? image : Uint8Array.from(image));
      }
      return { camera: cam, image, width, height };
    });
    return bakeTextureFromViews(device, mesh, views, options);
  } finally {
    device.synchronize();
    owned.forEach((b) => b.destroy());
  }
}
/** A uniform grid over `points` ([M*3] Float32Array, or a HipBuffer) for exact nearest-point queries under a cutoff (wdgs_point_index).  options:
 *  { cellSize, count }.  cellSize is a speed parameter only -- no result depends on it; without one it is chosen by the first query (its cutoff, or less
 *  for many points), which then finishes the build.  Non-finite points are left out.  The build waits once; queries are stream-ordered. */
class PointIndex {
  constructor(device, points, options) {
    const o = options || {};
    this.device = device; this.destroyed = false;
    const p = asDevice(device, points, Float32Array, 3, 'PointIndex: points');
    this.points = p.buf; this.owned = p.owned;
    this.numPoints = o.count === undefined || o.count === null ? p.rows : o.count;
    if (this.numPoints > p.rows) throw new Error('PointIndex: the count exceeds the buffer');
    this.handle = addon.pointIndexCreate(device.handle, this.points.ptr, this.numPoints, o.cellSize === undefined || o.cellSize === null ? 0 : o.cellSize);
  }
  /** { cellSize, dims, indexed }: the cell edge in use (0 before the first query of an index made without one), the grid, the finite points. */
  info() { const a = addon.pointIndexInfo(this.handle); return { cellSize: a[0], dims: [a[1], a[2], a[3]], indexed: a[4] }; }
  /** Room for queries of `count` points: what a recorded nearestInto needs beforehand (an eager query makes its own). */
  reserveQueries(count) { addon.pointIndexReserveQueries(this.handle, count); }
  /** Stream-ordered nearest: for the first `count` points of `queries` the squared distance (f32) to the nearest indexed point within maxDistance into
   *  d2 and that point's index into index -- the lowest index among equally near ones; +inf and 0xFFFFFFFF when there is none or the query is not finite.
   *  pairs (optional, 8 bytes): the number of pairs examined is added to it.  No host wait; records. */
  nearestInto(encoder, queries, count, maxDistance, d2, index, pairs) {
    if (queries.size < 12 * count || d2.size < 4 * count || index.size < 4 * count || (pairs && pairs.size < 8)) throw new Error(`PointIndex.nearest: buffers too small for ${count} queries`);
    addon.pointIndexNearest(this.handle, queries.ptr, count, maxDistance, d2.ptr, index.ptr, pairs ? pairs.ptr : null);
  }
  /** { d2: Float32Array[K], index: Uint32Array[K] } for `queries` ([K*3] Float32Array or a HipBuffer).  Synchronises. */
  nearest(queries, maxDistance) {
    const q = asDevice(this.device, queries, Float32Array, 3, 'PointIndex.nearest: queries'), k = q.rows;
    const d2 = this.device.createBuffer({ size: 4 * Math.max(k, 1) }), index = this.device.createBuffer({ size: 4 * Math.max(k, 1) });
    try {
      this.nearestInto(null, q.buf, k, maxDistance, d2, index);
      const bytes = (b, n) => (n ? this.device.readBuffer(b, n) : new ArrayBuffer(0));
      return { d2: new Float32Array(bytes(d2, 4 * k)), index: new Uint32Array(bytes(index, 4 * k)) };
    } finally { d2.destroy(); index.destroy(); if (q.owned) q.buf.destroy(); }
  }
  /** { lo, hi }: the bounding box of the finite points (Float32Array[3] each; zeros when there is none).  No device work. */
  bounds() { const a = addon.pointIndexBounds(this.handle); return { lo: Float32Array.from(a.slice(0, 3)), hi: Float32Array.from(a.slice(3, 6)) }; }
  /** Stream-ordered kNearest: for each of the first `count` points of `queries` the k (1 to 16) nearest indexed points within maxDistance, ordered by
   *  (squared distance, index), into row i of d2 f32[count][k] and index u32[count][k]; slots beyond the candidates, and every slot of a non-finite
   *  query, hold +inf and 0xFFFFFFFF.  excludeSelf: query i leaves out the indexed point i (the self-query).  pairs (optional, 8 bytes): the number of
   *  pairs examined is added to it.  No host wait; records. */
  kNearestInto(encoder, queries, count, k, maxDistance, d2, index, excludeSelf, pairs) {
    if (!(k >= 0 && k <= 0xFFFFFFFF) || queries.size < 12 * count || d2.size < 4 * count * k || index.size < 4 * count * k || (pairs && pairs.size < 8)) {
      throw new Error(`PointIndex.kNearest: buffers too small for ${count} queries with k = ${k}`);
    }
    addon.pointIndexKNearest(this.handle, queries.ptr, count, k, maxDistance, excludeSelf ? KNN_EXCLUDE_SELF : 0, d2.ptr, index.ptr, pairs ? pairs.ptr : null);
  }
  /** { d2: Float32Array[K*k], index: Uint32Array[K*k] }, row-major, for `queries` ([K*3] Float32Array or a HipBuffer).  Synchronises. */
  kNearest(queries, k, maxDistance, excludeSelf) {
    const q = asDevice(this.device, queries, Float32Array, 3, 'PointIndex.kNearest: queries'), n = q.rows;
    const room = 4 * Math.max(n * Math.max(0, Math.min(k, 1024)), 1);   // (the library refuses a k outside [1, 16])
    const d2 = this.device.createBuffer({ size: room }), index = this.device.createBuffer({ size: room });
    try {
      this.kNearestInto(null, q.buf, n, k, maxDistance, d2, index, excludeSelf);
      const bytes = (b, len) => (len ? this.device.readBuffer(b, len) : new ArrayBuffer(0));
      return { d2: new Float32Array(bytes(d2, 4 * n * k)), index: new Uint32Array(bytes(index, 4 * n * k)) };
    } finally { d2.destroy(); index.destroy(); if (q.owned) q.buf.destroy(); }
  }
  destroy() {
    if (this.destroyed) return;
    this.destroyed = true;
    addon.pointIndexDestroy(this.handle);
    this.handle = null;
    if (this.owned) this.points.destroy();
    this.points = null;
  }
}
/** 3DGS's scale initialisation, in place: every point of `pointCloud` gets log sigma = 0.5 log(max(mean, minD2)) on all three axes, mean the mean squared
 *  distance to its k nearest other points within maxDistance (fewer when fewer are there; a point without any keeps its scales).  The distances are those
 *  of the records' fp16 positions.  options: { k = 3, maxDistance (default: twice the widest extent of the finite positions, every other point a candidate;
 *  for a cloud with far outliers pass a cutoff), minD2 = 1e-7, count }.  Only halves 8, 9, 10 of each record of gaussian_3d_buffer change.  Returns
 *  { meanD2: Float32Array[N] (+inf without a neighbour), found: Uint32Array[N] }.  Synchronises. */
function initScalesFromNeighbours(device, pointCloud, options) {
  const o = options || {};
  const n = o.count === undefined || o.count === null ? pointCloud.num_points : o.count;
  if (n < 0 || n > pointCloud.num_points) throw new Error('initScalesFromNeighbours: the count exceeds the point cloud');
  const k = o.k === undefined || o.k === null ? 3 : o.k, minD2 = o.minD2 === undefined || o.minD2 === null ? 1e-7 : o.minD2;
  const g = pointCloud.gaussian_3d_buffer, slots = n * Math.max(0, Math.min(k, 1024));
  const positions = device.createBuffer({ size: 12 * Math.max(n, 1) }), d2 = device.createBuffer({ size: 4 * Math.max(slots, 1) });
  const idx = device.createBuffer({ size: 4 * Math.max(slots, 1) }), mean = device.createBuffer({ size: 4 * Math.max(n, 1) });
  let index = null;
  try {
    addon.pointCloudPositions(device.handle, g.ptr, n, positions.ptr);
    index = new PointIndex(device, positions, { count: n });
    let maxDistance = o.maxDistance;
    if (maxDistance === undefined || maxDistance === null) {
      const b = index.bounds();
      const widest = Math.max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]);
      maxDistance = widest > 0 ? 2 * widest : 1;
    }
    index.kNearestInto(null, positions, n, k, maxDistance, d2, idx, true);
    addon.pointCloudNeighbourScales(device.handle, g.ptr, n, d2.ptr, k, minD2, mean.ptr);
    const bytes = (b, len) => (len ? device.readBuffer(b, len) : new ArrayBuffer(0));
    const rows = new Float32Array(bytes(d2, 4 * n * k)), found = new Uint32Array(n);
    for (let i = 0; i < n; i++) for (let s = 0; s < k; s++) if (Number.isFinite(rows[i * k + s])) found[i]++;
    return { meanD2: new Float32Array(bytes(mean, 4 * n)), found };
  } finally {
    if (index) index.destroy();
    positions.destroy(); d2.destroy(); idx.destroy(); mean.destroy();
  }
}
/** Stream-ordered pointDistanceStats: the three u64 sums into the first 24 bytes of `out` (no host wait). */
function encodePointDistanceStats(device, d2, count, maxDistance, threshold, out) {
  if (d2.size < 4 * count || out.size < 24) throw new Error(`pointDistanceStats: buffers too small for ${count} distances`);
  addon.pointDistanceStats(device.handle, d2.ptr, count, maxDistance, threshold, out.ptr);
}
/** Exact integer statistics of PointIndex.nearest's squared distances (a Float32Array, or a HipBuffer with `count`): { n, n_found (finite), n_within
 *  (d2 <= threshold^2), sum_q (the sum of u32(sqrt(d2) / maxDistance 2^24) over the found; a Number, exact below 2^53), mean = sum_q maxDistance / 2^24 /
 *  n_found (NaN when nothing was found) }.  0 < threshold <= maxDistance.  Synchronises. */
function pointDistanceStats(device, d2, maxDistance, threshold, count) {
  const d = d2 instanceof HipBuffer ? { buf: d2, rows: count === undefined || count === null ? Math.floor(d2.size / 4) : count, owned: false }
    : asDevice(device, d2, Float32Array, 1, 'pointDistanceStats: d2');
  const out = device.createBuffer({ size: 24 });
  try {
    encodePointDistanceStats(device, d.buf, d.rows, maxDistance, threshold, out);
    const v = new BigUint64Array(device.readBuffer(out, 24));
    const found = Number(v[0]), sum = Number(v[2]);
    return { n: d.rows, n_found: found, n_within: Number(v[1]), sum_q: sum, mean: found ? sum * Math.fround(maxDistance) / 2 ** 24 / found : NaN };
  } finally { out.destroy(); if (d.owned) d.buf.destroy(); }
}
/** How far a point set is from a reference set, in both directions: accuracy the mean distance from `points` to their nearest `reference` point over
 *  the points that have one within maxDistance (the others are outliers: counted, not averaged), completeness the same from the reference to the points,
 *  chamfer their mean, precision / recall the share of points / reference points within `threshold`, fscore = 2PR / (P + R) (0 when both are 0); a
 *  direction with nothing found gives NaN.  Both sets: [N*3] Float32Array or HipBuffer (options: { numPoints, numReference } for buffers used in part). */
function geometryMetrics(device, points, reference, maxDistance, threshold, options) {
  const o = options || {};
  const p = asDevice(device, points, Float32Array, 3, 'geometryMetrics: points'), r = asDevice(device, reference, Float32Array, 3, 'geometryMetrics: reference');
  const np = o.numPoints === undefined || o.numPoints === null ? p.rows : o.numPoints, nr = o.numReference === undefined || o.numReference === null ? r.rows : o.numReference;
  const room = 4 * Math.max(np, nr, 1);
  const d2 = device.createBuffer({ size: room }), idx = device.createBuffer({ size: room }), out = device.createBuffer({ size: 48 });
  const indices = [];
  let s;
  try {
    [[p.buf, np, r.buf, nr], [r.buf, nr, p.buf, np]].forEach(([src, nSrc, dst, nDst], k) => {
      const index = new PointIndex(device, dst, { count: nDst });
      indices.push(index);
      index.nearestInto(null, src, nSrc, maxDistance, d2, idx);
      addon.pointDistanceStats(device.handle, d2.ptr, nSrc, maxDistance, threshold, out.ptr + BigInt(24 * k));
    });
    s = Array.from(new BigUint64Array(device.readBuffer(out, 48)), Number);
  } finally {
    for (const index of indices) index.destroy();
    d2.destroy(); idx.destroy(); out.destroy();
    if (p.owned) p.buf.destroy();
    if (r.owned) r.buf.destroy();
  }
  const scale = Math.fround(maxDistance) / 2 ** 24;
  const accuracy = s[0] ? s[2] * scale / s[0] : NaN, completeness = s[3] ? s[5] * scale / s[3] : NaN;
  const precision = np ? s[1] / np : NaN, recall = nr ? s[4] / nr : NaN;
  return { accuracy, completeness, chamfer: (accuracy + completeness) / 2, precision, recall,
    fscore: precision === 0 && recall === 0 ? 0 : 2 * precision * recall / (precision + recall),
    n_points: np, n_reference: nr, outliers_points: np - s[0], outliers_reference: nr - s[3] };
}

/** The normals of an f32 depth image by central differences of its back-projection (loaders.backprojectDepth's convention): rgba32f { n, 1 } into
 *  `target`, all zero where a neighbour is missing (wdgs_depth_to_normals).  `camera`: the 68-float block, or [proj[0][0], proj[1][1]].
 *  Stream-ordered; no reference counterpart. */
function depthToNormals(device, depth, width, height, camera, target) {
  if (depth.size < 4 * width * height || target.size < 16 * width * height) throw new Error(`depthToNormals: buffers too small for ${width}x${height}`);
  const p = camera.length === 68 ? [camera[32], camera[37]] : [camera[0], camera[1]];
  addon.depthToNormals(device.handle, depth.ptr, width, height, p[0], p[1], target.ptr);
}
/** Stream-ordered normalAgreement: the three u64 sums into the first 24 bytes of `out` (no host wait). */
function encodeNormalAgreement(device, normal, depthNormals, width, height, out) {
  if (normal.size < 16 * width * height || depthNormals.size < 16 * width * height || out.size < 24) throw new Error(`normalAgreement: buffers too small for ${width}x${height}`);
  addon.normalAgreement(device.handle, normal.ptr, depthNormals.ptr, width, height, out.ptr);
}
/** How well a composited normal image (getNormalTextureView) agrees with a depth-normal image (depthToNormals), over the pixels with A >= 0.5, |N| > 0
 *  and a valid depth normal: { sum_e, sum_a, pixels } (exact integer sums of rint(A (1 - cos) 2^24) and rint(A 2^24), as Numbers: below 2^53 for any
 *  image) and value = sum_e / sum_a, the weight-averaged 1 - cos (NaN when nothing counts).  Synchronises.  No reference counterpart. */
function normalAgreement(device, normal, depthNormals, width, height) {
  const out = device.createBuffer({ size: 24 });
  try {
    encodeNormalAgreement(device, normal, depthNormals, width, height, out);
    const v = new BigUint64Array(device.readBuffer(out, 24));
    const e = Number(v[0]), a = Number(v[1]);
    return { sum_e: e, sum_a: a, pixels: Number(v[2]), value: a ? e / a : NaN };
  } finally { out.destroy(); }
}
/** A normal image as rgba8 for presentation: round(255 (0.5 + 0.5 (n_x, -n_y, -n_z))) of the normalised normal (facing the camera: blue), black where
 *  |N| = 0, alpha 255 (wdgs_normal_to_rgba8).  Stream-ordered; no reference counterpart. */
function normalToRGBA8(device, normal, width, height, target) {
  if (normal.size < 16 * width * height || target.size < 4 * width * height) throw new Error(`normalToRGBA8: buffers too small for ${width}x${height}`);
  addon.normalToRgba8(device.handle, normal.ptr, width, height, target.ptr);
}

/** One zeroed 16-byte record { u64 sum_q; u32 max_bits; u32 pixels } per Gaussian, for TiledRasterizer.encodeContribution.  No reference counterpart. */
function createContributionBuffer(device, numPoints) {
  const buf = device.createBuffer({ size: CONTRIBUTION_RECORD_BYTES * Math.max(1, numPoints), label: 'contribution' });
  addon.bufferClear(device.handle, buf.ptr, buf.size);
  return buf;
}
/** The first n records: { sum_q: BigUint64Array, weight_sum: Float64Array (sum_q * 2^-24), max_weight: Float32Array, pixels: Uint32Array }. */
function readContribution(buffer, n) {
  const raw = buffer.device.readBuffer(buffer, CONTRIBUTION_RECORD_BYTES * n);
  const q = new BigUint64Array(raw), w = new Uint32Array(raw);
  const out = { sum_q: new BigUint64Array(n), weight_sum: new Float64Array(n), max_weight: new Float32Array(n), pixels: new Uint32Array(n) };
  const bits = new Uint32Array(out.max_weight.buffer);
  for (let i = 0; i < n; i++) {
    out.sum_q[i] = q[2 * i]; out.weight_sum[i] = Number(q[2 * i]) * 2 ** -24;   // (sum_q < 2^53: exact)
    bits[i] = w[4 * i + 2]; out.pixels[i] = w[4 * i + 3];
  }
  return out;
}

/** The C-ABI communicator (wdgs_comm_*, include/webdgs.h): RCCL queued on the device's stream by the library itself -- the transport of the
 *  data-parallel step for a host without torch.distributed.  `uniqueId` (ArrayBuffer, 128 bytes) comes from Communicator.uniqueId() on rank 0 and
 *  reaches the other ranks over any host channel (parallel.js ships it through a file). */
class Communicator {
  constructor(device, uniqueId, worldSize, rank) {
    this.device = device; this.worldSize = worldSize; this.rank = rank;
    this.handle = addon.commCreate(device.handle, uniqueId, worldSize, rank);
  }
  static uniqueId() { return addon.commUniqueId(); }
  exchangeGradients(grad, visible, flag, slicePoints) { addon.commExchangeGradients(this.handle, grad.ptr, visible.ptr, flag ? flag.ptr : null, slicePoints); }
  allgatherRows(rows, slicePoints) { addon.commAllgatherRows(this.handle, rows.ptr, slicePoints); }
  broadcast(ptr, bytes, root) { addon.commBroadcast(this.handle, ptr, bytes, root); }
  allreduceCounts(counts, count) { addon.commAllreduceCounts(this.handle, counts.ptr, count); }
  allreduceGradients(grad, visible, numPoints) { addon.commAllreduceGradients(this.handle, grad.ptr, visible.ptr, numPoints); }
  static groupStart() { addon.commGroup(0); }
  static groupEnd() { addon.commGroup(1); }
  destroy() { if (this.handle !== null) { addon.commDestroy(this.handle); this.handle = null; } }
}

const MAX_LANES = 4;         // WDGS_MAX_LANES
const MAX_BATCH_VIEWS = 16;  // WDGS_MAX_BATCH_VIEWS

module.exports = { addon, DEPTH_KINDS, depthToRGBA8, TSDFVolume, weldTriangles, MeshWelder, weldTrianglesDevice, destroyBuffers, MeshSimplifier, simplifyMesh, MeshAdjacency, meshAdjacency, smoothMesh, vertexNormals, finishMesh, CULL_MODES, MESH_RASTER_LARGE_FACE_PIXELS, MESH_RASTER_NEAR, NO_FACE, MeshRasterizer, rasterizeMesh, encodeDepthAgreement, depthAgreementResult, depthAgreement, meshOnDevice, NO_INDEX, KNN_EXCLUDE_SELF, MeshSampler, sampleMesh, MeshComponents, meshComponents, selectComponents, removeSmallComponents, PointIndex, initScalesFromNeighbours, encodePointDistanceStats, pointDistanceStats,
  geometryMetrics, NO_NORMAL, depthToNormals, encodeNormalAgreement, normalAgreement, normalToRGBA8, CONTRIBUTION_RECORD_BYTES, createContributionBuffer, readContribution, MAX_LANES, MAX_BATCH_VIEWS, projectViews, geometryViews, imageSSE, imagePSNR, imageSSIM, encodeImageSSE, encodeImageSSIM, psnrFromSSE, Communicator, HipBuffer, HipCommandBuffer, HipEncoder, HipDevice, CapacityReports, grownTileEntries, allocatePointCloudLike, PrefixScanner, get_prefix_scanner, DynamicSortStuff,
  get_dynamic_sorter, TiledForwardPass, TiledRasterizer, TiledBackwardPass, DEFAULT_ADAM_HYPERPARAMETERS, allocateOptimizerStateBuffers, Optimizer,
  DensifyPrunePass, downsampleRGBA8, FaceVisibility, MeshFaceFilter, encodeFaceVisibilityFlags, selectFaces, filterFaces, faceVisibility, gatherVertexAttributes,
  MeshColourBaker, bakeMeshFromViews, bakeVertexColours, MeshTextureBaker, textureLayout, bakeTextureFromViews, bakeTexture };
