// Typings of webdgs_hip.js: the reference's operator classes (src/renderers/*.ts, src/sort/sort_dynamic.ts, src/prefix/prefix.ts,
// src/utils/allocate-pointcloud.ts) with GPUDevice / GPUBuffer / GPUTextureView / GPUCommandEncoder replaced by Hip* handle types.
export type RenderMode = 'gaussian' | 'pointcloud';

export class HipBuffer {
  readonly device: HipDevice; readonly ptr: bigint; readonly size: number; destroyed: boolean;
  /** Called before the buffer's content is handed to the host or copied by copyBufferToBuffer (deferred SH writes, the compact training copy). */
  beforeRead: (() => void) | null;
  read(byteLength?: number): ArrayBuffer;
  destroy(): void;
}
export class HipCommandBuffer { readonly device: HipDevice; destroy(): void; }
export class HipEncoder {
  readonly device: HipDevice; readonly label: string; readonly record: boolean;
  clearBuffer(buffer: HipBuffer): void;
  copyBufferToBuffer(src: HipBuffer, srcOffset: number, dst: HipBuffer, dstOffset: number, size: number): void;
  finish(): HipCommandBuffer;
  abort(): void;
}
// capacity reports and the growth rule of tile-entry lists live in capacity_reports.js (no addon needed) and are re-exported here
import { CapacityReports } from './capacity_reports';
export { CapacityReports, Overflow, Settled, grownTileEntries } from './capacity_reports';
export class HipDevice {
  constructor(ordinal?: number);
  readonly capacityReports: CapacityReports;
  readonly queue: {
    submit(cmds: HipCommandBuffer[]): void;
    onSubmittedWorkDone(): Promise<void>;
    /** include/webdgs.h wdgs_queue_mark / wdgs_queue_wait: keep the completion of step k and await it after submitting step k+1. */
    mark(): number;
    wait(ticket: number): void;
    writeBuffer(buffer: HipBuffer, offset: number, data: ArrayBufferView | ArrayBuffer): void;
  };
  createBuffer(desc: { size: number; label?: string }): HipBuffer;
  createCommandEncoder(desc?: { label?: string; record?: boolean }): HipEncoder;
  view(ptr: bigint, size: number): HipBuffer;
  readBuffer(buffer: HipBuffer, byteLength?: number): ArrayBuffer;
  createPinnedArrayBuffer(byteLength: number): ArrayBuffer;
  readBufferAsync(buffer: HipBuffer, offset: number, pinned: ArrayBuffer, byteLength: number): Promise<ArrayBuffer>;
  synchronize(): void;
  /** device.limits as far as memory goes (trainer.ts:147): bytes; `cached` is what the library's allocation cache holds. */
  memoryInfo(): { free: number; total: number; cached: number };
  /** Lanes (include/webdgs.h): lane 0 is the device's stream, 1..3 internal ones; work on different lanes may overlap. */
  selectLane(lane: number): void;
  laneOrder(waiterLane: number, signalLane: number): void;
  laneMark(lane: number, mark: number): void;
  laneWaitMark(lane: number, mark: number): void;
  /** Per-kernel hipEvent timing (wdgs_device_set_profiling / wdgs_device_get_kernel_times). */
  setProfiling(enabled: boolean): void;
  kernelTimes(reset?: boolean): { [kernel: string]: { launches: number; totalMs: number } };
  destroy(): void;
}
export const MAX_LANES: number;
export const MAX_BATCH_VIEWS: number;

export interface PointCloud {          // src/utils/load-pointcloud.ts:16-23
  type: 'full' | 'normal'; num_points: number; sh_deg?: number; gaussian_3d_buffer: HipBuffer; sh_buffer?: HipBuffer;
  /** Set while an Optimizer trains this cloud with deferred SH writes: the compact SH-DC array forward passes built on the cloud read. */
  dcWords?: HipBuffer | null;
}
export function allocatePointCloudLike(device: HipDevice, template: PointCloud, options: { numPoints: number }): PointCloud;

export class PrefixScanner {             // src/prefix/prefix.ts:26-43
  readonly input_buffer: HipBuffer; readonly output_buffer: HipBuffer; readonly max_elements: number;
  set_count(count: number): { num_workgroups: number };
  scan(encoder: HipEncoder | null): void;
  destroy(): void;
}
export function get_prefix_scanner(maxElements: number, device: HipDevice): PrefixScanner;
export class DynamicSortStuff {          // src/sort/sort_dynamic.ts:9-24
  readonly capacity: number; final_out_index: number;
  readonly ping_pong: { sort_depths_buffer: HipBuffer; sort_indices_buffer: HipBuffer }[];
  sort(encoder: HipEncoder | null, keyBits?: number): void;
  destroy(): void;
}
export function get_dynamic_sorter(maxCapacity: number, device: HipDevice, statsBuffer: HipBuffer): DynamicSortStuff;

export interface TiledForwardPassConfig {  // tiled-forward-pass.ts:24-31
  viewportWidth: number; viewportHeight: number; gaussianScale?: number; pointSizePx?: number; maxSplatRadiusPx?: number; renderMode?: RenderMode;
  maxTileEntries?: number; compatCaps?: boolean;
}
export interface TiledForwardResources {   // tiled-forward-pass.ts:33-46
  splatBuffer: HipBuffer; tileKeysBuffer: HipBuffer; tileIndicesBuffer: HipBuffer; tileOffsetsBuffer: HipBuffer; tileCountsBuffer: HipBuffer;
  statsBuffer: HipBuffer; numTilesX: number; numTilesY: number; totalTiles: number; maxTileEntries: number;
}
export class TiledForwardPass {
  constructor(device: HipDevice, pointCloud: PointCloud, cameraBuffer: HipBuffer, config: TiledForwardPassConfig);
  readonly nativeHandle: bigint;
  encode(encoder: HipEncoder | null, options?: { skipSort?: boolean }): void;
  setCameraBuffer(buffer: HipBuffer): void;
  /** Resize instead of rebuild (include/webdgs.h wdgs_tiled_forward_resize); false if the SH degree differs. */
  setPointCloud(pointCloud: PointCloud): boolean;
  /** K1 takes the SH-DC halves from the optimizer's compact array (Optimizer.setDeferredSH); null restores the rows. */
  setDcSource(dcWords: HipBuffer | null): void;
  /** Follows pointCloud.dcWords (called by encode / projectViews): a pass built on a cloud in training renders the trained colours by itself. */
  syncDcSource(): void;
  /** The rest of encode (scan, emit, sort) after projectViews ran K1 for this pass (view-batched step; no reference counterpart). */
  encodeProjected(encoder: HipEncoder | null): void;
  isProjected(): boolean;
  setRenderMode(mode: RenderMode): void; setPointSize(value: number): void; setGaussianScale(value: number): void; setViewport(width: number, height: number): void;
  getResources(): TiledForwardResources;
  getSortedIndicesBuffer(): HipBuffer; getSortedKeysBuffer(): HipBuffer; getTileOffsetsBuffer(): HipBuffer; getStatsBuffer(): HipBuffer;
  check(): { totalTileEntries: number; visibleCount: number };
  setLongLists(threshold: number, maxItems?: number, maxRows?: number): void;
  longListStats(): { blocksWanted: number; itemsWanted: number; forwardQueue: number; backwardQueue: number; rowsUsed: number; rowsWanted: number; stalled: number; maxItems: number; maxBlocks: number; maxRows: number; threshold: number };
  destroy(): void;
}
export type DepthKind = 'expected' | 'median' | 'weight_sum';
export const DEPTH_KINDS: { expected: 1; median: 2; weight_sum: 4 };
export class TiledRasterizer {
  constructor(config: { device: HipDevice; forwardPass: TiledForwardPass; format?: string });
  encode(encoder: HipEncoder | null, width: number, height: number): void;
  getOutputTextureView(): HipBuffer; getAlphaTextureView(): HipBuffer; getNContribTextureView(): HipBuffer; getTileOffsetsBuffer(): HipBuffer;
  /** `target` may carry its own `width` / `height` (a canvas of another size); the clear colour is accepted for signature compatibility only. */
  /** Depth images of the frame the last encode rasterized (no reference counterpart); default kinds: ['expected']. */
  encodeDepth(encoder: HipEncoder | null, kinds?: DepthKind | DepthKind[] | number): void;
  /** Adds the per-Gaussian contribution of the frame the last encode rasterized into `statsBuffer` (no reference counterpart); records. */
  encodeContribution(encoder: HipEncoder | null, statsBuffer: HipBuffer): void;
  /** f32[W*H] of one kind the last encodeDepth wrote (default 'expected'). */
  getDepthTextureView(kind?: DepthKind): HipBuffer;
  /** The normal map of the frame the last encode rasterized (no reference counterpart): per-Gaussian view-space normals, composited with the colour's weights. */
  encodeNormal(encoder: HipEncoder | null): void;
  /** rgba32f[W*H] { N.x, N.y, N.z, A } of the last encodeNormal (N un-normalised: |N| <= A). */
  getNormalTextureView(): HipBuffer;
  /** u32[numPoints]: the packed per-Gaussian normals of the last encodeNormal (NO_NORMAL: none). */
  getGaussianNormals(): HipBuffer;
  blitToTexture(encoder: HipEncoder | null, target: HipBuffer & { width?: number; height?: number }, clearColor?: { r: number; g: number; b: number; a: number }): void;
  destroy(): void;
}
export interface TrainingConfig {  // tiled-backward-pass.ts:19-25
  lambda_l1: number; lambda_l2: number; lambda_dssim: number; c1?: number; c2?: number;
  /** The loss the backward pass differentiates (no reference counterpart): 'reference' (default) or 'gaussian', the exact 3DGS D-SSIM loss. */
  dssim_mode?: 'reference' | 'gaussian';
}
export interface TiledBackwardResources {  // tiled-backward-pass.ts:40-50
  splatBuffer: HipBuffer; tileOffsetsBuffer: HipBuffer; tileIndicesBuffer: HipBuffer; cameraBuffer?: HipBuffer; alphaTexture?: HipBuffer; nContribTexture: HipBuffer;
}
export class TiledBackwardPass {
  constructor(device: HipDevice, pointCloud: PointCloud, config: { viewportWidth: number; viewportHeight: number; trainingConfig: TrainingConfig; maxSplatRadiusPx?: number });
  encode(encoder: HipEncoder | null, predictedTexture: HipBuffer, targetTexture: HipBuffer, resources: TiledBackwardResources, options?: {}): void;
  /** The two halves of encode (a batched step; the fused single-view step): K15 + clear + K16, then K17. */
  encodeRaster(encoder: HipEncoder | null, predictedTexture: HipBuffer, targetTexture: HipBuffer, resources: TiledBackwardResources): void;
  encodeGeometry(encoder: HipEncoder | null, cameraBuffer: HipBuffer,
                 accumulate?: { sums: HipBuffer; visible: HipBuffer; tileCounts: HipBuffer; guard: HipBuffer; stats: HipBuffer; first: boolean } | null): void;
  /** Whether Optimizer.stepWithGeometry also writes K17's packed gradient to getGradientsBuffer() (default true, as the reference's K17 does). */
  setGradientOutput(enabled: boolean): void;
  /** computeMetricCounts adds into `counts` (another pass's metric counts) instead of this pass's own array; null restores its own. */
  setMetricCountsTarget(counts: HipBuffer | null): void;
  setTrainingConfig(next: Partial<TrainingConfig>): void;
  getMetricMapTexture(): HipBuffer;
  computeLossOnly(encoder: HipEncoder | null, predicted: HipBuffer, target: HipBuffer): void;
  computeMetricMap(encoder: HipEncoder | null, predicted: HipBuffer, target: HipBuffer, options?: { threshold?: number }): void;
  computeMetricCounts(encoder: HipEncoder | null, resources: TiledBackwardResources, options?: { clear?: boolean; numInstances?: number }): void;
  normalizeMetricCounts(encoder: HipEncoder | null, options: { divisor: number }): void;
  setViewport(width: number, height: number): void;
  /** Resize instead of rebuild (include/webdgs.h wdgs_tiled_backward_resize); false if the SH degree differs. */
  setPointCloud(pointCloud: PointCloud): boolean;
  getGradientsBuffer(): HipBuffer; getMetricCountsBuffer(): HipBuffer; getLossTextureView(): HipBuffer; getMetricMapTextureView(): HipBuffer;
  destroy(): void;
}
export interface AdamHyperparameters { lr_pos: number; lr_color: number; lr_opacity: number; lr_scale: number; lr_rot: number; beta1: number; beta2: number; epsilon: number; }
export const DEFAULT_ADAM_HYPERPARAMETERS: AdamHyperparameters;
export interface OptimizerStateBuffers {   // optimizer.ts:13-20
  optPosBuffer: HipBuffer; optRotBuffer: HipBuffer; optScaleBuffer: HipBuffer; optOpacityBuffer: HipBuffer; paramSH: HipBuffer; stateSH: HipBuffer;
}
export interface OptimizerInitialState { iteration: number; buffers: OptimizerStateBuffers; }   // optimizer.ts:22-25
export function allocateOptimizerStateBuffers(device: HipDevice, numPoints: number): OptimizerStateBuffers;
export class Optimizer {
  constructor(device: HipDevice, pointCloud: PointCloud, params?: Partial<AdamHyperparameters>, initialState?: OptimizerInitialState);
  getIteration(): number; getHyperparameters(): AdamHyperparameters; setHyperparameters(next: Partial<AdamHyperparameters>): void;
  getStateBuffers(): OptimizerStateBuffers;
  step(encoder: HipEncoder | null, coefficients: PointCloud, gradientsBuffer: HipBuffer, tileCountsBuffer: HipBuffer): void;
  /** Deferred SH writes (include/webdgs.h wdgs_optimizer_set_deferred_sh); no reference counterpart. */
  setDeferredSH(pointCloud: PointCloud, enabled?: boolean): HipBuffer | null;
  flushSH(pointCloud: PointCloud): void;
  setGuard(flagBuffer: HipBuffer | null, offset?: number): void;
  /** step() fused with K17 (wdgs_optimizer_step_with_geometry): after backwardPass.encodeRaster for the view. */
  stepWithGeometry(encoder: HipEncoder | null, coefficients: PointCloud, backwardPass: TiledBackwardPass, cameraBuffer: HipBuffer, tileCountsBuffer: HipBuffer): void;
  /** Data-parallel step (SURVEY 8(e)): Adam + re-pack on the owned slice; rowsOut receives the re-packed 32-byte rows. */
  stepF32Range(encoder: HipEncoder | null, coefficients: PointCloud, gradF32: HipBuffer, visibleCounts: HipBuffer, first: number, count: number, rowsOut?: HipBuffer | null): void;
  applyRepackedRows(rows: HipBuffer, skipFirst: number, skipCount: number, guard: HipBuffer | null, pointCloud: PointCloud): void;
  stateChanged(): void;
  advanceIteration(count?: number): void;
  destroy(): void;
}
export interface DensifyPruneConfig {      // densify-prune.ts:17-30
  strategy?: 'cpu_rebuild' | 'gpu_rebuild'; numViews?: number; cloneThreshold?: number; splitThreshold?: number; pruneThreshold?: number;
  maxNewPointsPerStep?: number; maxBufferBytes?: number;
}
export interface DensifyPrunePrepared {    // densify-prune.ts:42-48
  actionBuffer: HipBuffer; outCountBuffer: HipBuffer; outOffsetBuffer: HipBuffer; outTotalBuffer: HipBuffer; maxOutPoints: number;
}
export class DensifyPrunePass {
  constructor(device: HipDevice, config?: DensifyPruneConfig);
  setConfig(next: Partial<DensifyPruneConfig>): void; getConfig(): DensifyPruneConfig;
  ensureSize(numPoints: number): void; computeMaxOutPoints(pointCloud: PointCloud): number;
  encodeDecision(encoder: HipEncoder | null, inputs: { pointCloud: PointCloud; metricCountsBuffer?: HipBuffer }): { actionBuffer: HipBuffer; outCountBuffer: HipBuffer };
  /** Contribution-based pruning's decision (no reference counterpart): kept iff the record meets every non-zero field of the rule. */
  encodeContributionDecision(encoder: HipEncoder | null, numPoints: number, statsBuffer: HipBuffer, rule: ContributionRule): { actionBuffer: HipBuffer; outCountBuffer: HipBuffer };
  encodePrefixSum(encoder: HipEncoder | null): HipBuffer;
  encodeCapToMax(encoder: HipEncoder | null, outOffsetBuffer: HipBuffer, maxOutPoints: number): void;
  encodeTotalOut(encoder: HipEncoder | null, outOffsetBuffer: HipBuffer | null): HipBuffer;
  getActionBuffer(): HipBuffer | null;
  getOutCountBuffer(): HipBuffer | null;
  getOutTotalBuffer(): HipBuffer;
  encodePrepare(encoder: HipEncoder | null, inputs: { pointCloud: PointCloud; metricCountsBuffer?: HipBuffer }): DensifyPrunePrepared;
  readTotal(): number;
  encodeScatter(encoder: HipEncoder | null,
                inputs: { pointCloud: PointCloud; optimizerState?: OptimizerStateBuffers; outOffsetBuffer: HipBuffer; outNumPoints: number; resetNewOptimizerState?: boolean },
                outputs: { outPointCloud: PointCloud; outOptimizerState?: OptimizerStateBuffers }): void;
  applyActions(encoder: HipEncoder | null): never;
  destroy(): void;
}
export function downsampleRGBA8(device: HipDevice, src: HipBuffer, srcW: number, srcH: number, dst: HipBuffer, dstW: number, dstH: number): void;
/** View-batched K1 / K17 (include/webdgs.h wdgs_tiled_forward_project_views, wdgs_tiled_backward_encode_geometry_views); no reference counterpart. */
export function projectViews(forwardPasses: TiledForwardPass[], cameraBuffers: HipBuffer[], pointCloud: PointCloud): void;
export function geometryViews(backwardPasses: TiledBackwardPass[], cameraBuffers: HipBuffer[], forwardPasses: TiledForwardPass[], sums: HipBuffer, visible: HipBuffer, guard: HipBuffer,
                              pointCloud: PointCloud, writeGradients?: boolean, continues?: boolean): void;
export function imageSSE(device: HipDevice, a: HipBuffer, b: HipBuffer, numPixels: number): number;
export function imagePSNR(device: HipDevice, a: HipBuffer, b: HipBuffer, numPixels: number): number;
export function psnrFromSSE(sse: number | bigint, numPixels: number): number;
export function encodeImageSSE(device: HipDevice, a: HipBuffer, b: HipBuffer, numPixels: number, out: HipBuffer): void;
export function encodeImageSSIM(device: HipDevice, a: HipBuffer, b: HipBuffer, width: number, height: number, out: HipBuffer, map?: HipBuffer | null): void;
export interface ContributionRule { minMaxWeight?: number; minWeightSum?: number; minPixels?: number; minSumQ?: number | bigint }
export interface ContributionRecords { sum_q: BigUint64Array; weight_sum: Float64Array; max_weight: Float32Array; pixels: Uint32Array }
export const CONTRIBUTION_RECORD_BYTES: 16;
/** One zeroed record { u64 sum_q; u32 max_bits; u32 pixels } per Gaussian, for TiledRasterizer.encodeContribution.  No reference counterpart. */
export function createContributionBuffer(device: HipDevice, numPoints: number): HipBuffer;
export function readContribution(buffer: HipBuffer, n: number): ContributionRecords;
/** A depth image as rgba8 for presentation: inverse depth between near (white) and far (black), depth 0 black.  No reference counterpart. */
export function depthToRGBA8(device: HipDevice, depth: HipBuffer, width: number, height: number, near: number, far: number, target: HipBuffer): void;
export function imageSSIM(device: HipDevice, a: HipBuffer, b: HipBuffer, width: number, height: number, map?: HipBuffer | null): number;
export interface TSDFVolumeOptions { truncation?: number | null; maxWeight?: number | null; colour?: boolean | null }
export interface TSDFTriangles { positions: Float32Array; keys: BigUint64Array; colours: Uint8Array | null; count: number }
export interface TriangleMesh { vertices: Float32Array; faces: Uint32Array; colours: Uint8Array | null; keys?: BigUint64Array }
/** A device TSDF volume (wdgs_tsdf_volume): fuses depth maps view by view, extracts the zero level set by marching tetrahedra.  No reference counterpart. */
export class TSDFVolume {
  constructor(device: HipDevice, origin: ArrayLike<number>, voxelSize: number, dims: ArrayLike<number>, options?: TSDFVolumeOptions);
  static fromBounds(device: HipDevice, lo: ArrayLike<number>, hi: ArrayLike<number>, voxelSize: number, options?: TSDFVolumeOptions): TSDFVolume;
  readonly origin: Float32Array; readonly voxelSize: number; readonly dims: number[]; readonly truncation: number; readonly maxWeight: number;
  readonly colour: boolean; readonly numVoxels: number;
  getTSDFBuffer(): HipBuffer;
  getWeightBuffer(): HipBuffer;
  getColourBuffer(): HipBuffer;
  reset(): void;
  integrate(depth: HipBuffer, camera: HipBuffer, width: number, height: number,
            options?: { weightSum?: HipBuffer | null; colour?: HipBuffer | null; minWeightSum?: number | null }): void;
  countTriangles(minWeight?: number | null): number;
  extractTriangles(minWeight?: number | null): TSDFTriangles;
  /** extractTriangles without the read-back: what weldTrianglesDevice takes; the caller destroys the buffers (destroyBuffers). */
  extractTriangleBuffers(minWeight?: number | null): TSDFTriangleBuffers;
  /** weld: 'host' (default: weldTriangles) or 'device' (weldTrianglesDevice: the same bytes, slot-sized arrays never cross the bus). */
  extractMesh(minWeight?: number | null, options?: { weld?: 'host' | 'device'; simplify?: null }): TriangleMesh;
  /** simplify: a cell size -- the welded mesh goes through simplifyMesh on that grid from the volume's origin (with weld 'device', on the device). */
  extractMesh(minWeight: number | null | undefined, options: { weld?: 'host' | 'device'; simplify: number }): SimplifiedMesh;
  /** smooth: an iteration count -- smoothMesh with its defaults, before simplify, with stats added; normals: vertexNormals of the final mesh is added. */
  extractMesh(minWeight: number | null | undefined, options: { weld?: 'host' | 'device'; simplify?: number | null; smooth?: number | null; normals?: boolean }):
    TriangleMesh & { stats?: AdjacencyStats | SimplifyStats; normals?: Float32Array; faceMap?: Uint32Array; vertexCluster?: Uint32Array };
  destroy(): void;
}
/** extractTriangles' output as an indexed mesh: vertices are the distinct edge keys in ascending order.  No reference counterpart. */
export function weldTriangles(tri: TSDFTriangles): TriangleMesh;
/** positions f32[F][3][3], keys u64[F][3], colours rgba8[F][3] on the device. */
export interface TSDFTriangleBuffers { positions: HipBuffer; keys: HipBuffer; colours: HipBuffer | null; numTriangles: number }
/** vertices f32[V][3], faces u32[F][3], keys u64[V], colours rgba8[V] on the device, each buffer of exactly that size. */
export interface WeldedMeshBuffers { vertices: HipBuffer; faces: HipBuffer; colours: HipBuffer | null; keys: HipBuffer; numVertices: number; numFaces: number }
/** Welds a triangle soup on the device (wdgs_mesh_welder): a stable u64 radix sort of (key, slot) pairs, head flags, a scan, a gather; count, then emit with
 *  the same keys.  No reference counterpart. */
export class MeshWelder {
  constructor(device: HipDevice);
  readonly numSlots: number; readonly numVertices: number;
  count(keys: HipBuffer | null, numSlots: number): number;
  emit(keys: HipBuffer | null, numSlots: number, positions: HipBuffer | null, colours: HipBuffer | null, facesOut: HipBuffer | null, verticesOut?: HipBuffer | null,
       coloursOut?: HipBuffer | null, keysOut?: HipBuffer | null, capacity?: number | null): void;
  stats(): { passesRun: number; passesSkipped: number; vertices: number; slots: number };
  destroy(): void;
}
/** weldTriangles on the device, byte for byte; a vertex takes the position and colour of the lowest slot that carries its key.  No reference counterpart. */
export function weldTrianglesDevice(device: HipDevice, tri: TSDFTriangles | TSDFTriangleBuffers, options?: { asBuffers?: false }): TriangleMesh;
export function weldTrianglesDevice(device: HipDevice, tri: TSDFTriangles | TSDFTriangleBuffers, options: { asBuffers: true }): WeldedMeshBuffers;
/** Destroys every HipBuffer among the values of `buffers`. */
export function destroyBuffers(buffers: object): void;
/** The last count of a MeshSimplifier: the occupied cells, the dropped faces by class, V' and F'. */
export interface SimplifyStats { clusters: number; invalid: number; outside: number; collapsed: number; duplicate: number; vertices: number; faces: number }
/** A simplified mesh: keys are the vertices' cell keys, faceMap the old face of each new one, vertexCluster the new vertex of each old one (0xFFFFFFFF: none). */
export interface SimplifiedMesh extends TriangleMesh { faceMap: Uint32Array; vertexCluster: Uint32Array; stats: SimplifyStats }
/** The same on the device, each buffer of exactly its size: f32[V'][3], u32[F'][3], rgba8[V'], u64[V'], u32[F'], u32[V]. */
export interface SimplifiedMeshBuffers { vertices: HipBuffer; faces: HipBuffer; colours: HipBuffer | null; keys: HipBuffer; faceMap: HipBuffer; vertexCluster: HipBuffer;
                                         numVertices: number; numFaces: number; stats: SimplifyStats }
/** A mesh on the device: f32[V][3], u32[F][3], rgba8[V]; without the counts, whole buffers. */
export interface MeshBuffers { vertices: HipBuffer; faces: HipBuffer; colours?: HipBuffer | null; numVertices?: number; numFaces?: number }
/** Simplifies an indexed mesh on the device by vertex clustering (wdgs_mesh_simplifier): cell keys, the weld's stable sort, integer means per cluster, the
 *  face filter; count, then emit with the same mesh.  No reference counterpart. */
export class MeshSimplifier {
  constructor(device: HipDevice);
  readonly numVertices: number; readonly numFaces: number;
  count(vertices: HipBuffer | null, numVertices: number, faces: HipBuffer | null, numFaces: number, colours: HipBuffer | null, origin: ArrayLike<number>,
        cellSize: number): { vertices: number; faces: number };
  emit(vertices: HipBuffer | null, numVertices: number, faces: HipBuffer | null, numFaces: number, colours: HipBuffer | null, verticesOut: HipBuffer | null,
       facesOut: HipBuffer | null, coloursOut?: HipBuffer | null, keysOut?: HipBuffer | null, faceMap?: HipBuffer | null, vertexCluster?: HipBuffer | null,
       capacityVertices?: number | null, capacityFaces?: number | null): void;
  stats(): SimplifyStats;
  destroy(): void;
}
/** `mesh` simplified by vertex clustering on a grid of cellSize from options.origin (default, typed-array input only: the minimum of the finite vertices);
 *  a function of its arguments alone, bit for bit.  No reference counterpart. */
export function simplifyMesh(device: HipDevice, mesh: { vertices: Float32Array; faces: Uint32Array; colours?: Uint8Array | null } | MeshBuffers, cellSize: number,
                             options?: { origin?: ArrayLike<number> | null; asBuffers?: false }): SimplifiedMesh;
export function simplifyMesh(device: HipDevice, mesh: { vertices: Float32Array; faces: Uint32Array; colours?: Uint8Array | null } | MeshBuffers, cellSize: number,
                             options: { origin?: ArrayLike<number> | null; asBuffers: true }): SimplifiedMeshBuffers;
/** The last count of a MeshAdjacency: E and E / 2, the undirected edges that one face (boundary) or three and more (non-manifold) hold, the faces left out,
 *  the ends of boundary edges, the vertices without a neighbour, the longest row. */
export interface AdjacencyStats { directedEdges: number; edges: number; boundaryEdges: number; nonManifoldEdges: number; invalidFaces: number; boundaryVertices: number;
                                  isolatedVertices: number; maxDegree: number }
export interface SmoothOptions { lambda?: number; mu?: number; pinBoundary?: boolean }
/** The per-vertex neighbour lists of an indexed mesh on the device (wdgs_mesh_adjacency): one stable u64 sort of the faces' directed half-edge keys; count, then
 *  emit, smooth (Taubin's lambda | mu steps) and normals (area-weighted) over that count.  No reference counterpart. */
export class MeshAdjacency {
  constructor(device: HipDevice);
  readonly numEdges: number; readonly numVertices: number; readonly numFaces: number;
  count(faces: HipBuffer | null, numFaces: number, numVertices: number): number;
  emit(rowStart?: HipBuffer | null, neighbours?: HipBuffer | null, boundary?: HipBuffer | null, capacityEdges?: number | null): void;
  smooth(verticesIn: HipBuffer | null, verticesOut: HipBuffer | null, numVertices: number, iterations?: number | null, options?: SmoothOptions): void;
  normals(vertices: HipBuffer | null, faces: HipBuffer | null, numVertices: number, numFaces: number, normalsOut: HipBuffer | null): void;
  stats(): AdjacencyStats;
  destroy(): void;
}
export type MeshArrays = { vertices: Float32Array; faces: Uint32Array; colours?: Uint8Array | null };
/** rowStart[V + 1], neighbours[E] (ascending within a row) and boundary[V] of the mesh's faces; a function of the faces alone, bit for bit. */
export function meshAdjacency(device: HipDevice, mesh: MeshArrays | MeshBuffers): { rowStart: Uint32Array; neighbours: Uint32Array; boundary: Uint32Array; stats: AdjacencyStats };
/** `mesh` after `iterations` (default 10) rounds of Taubin smoothing: its object with new vertices and stats added; bit for bit a function of its arguments. */
export function smoothMesh<M extends MeshArrays>(device: HipDevice, mesh: M, iterations?: number | null, options?: SmoothOptions & { asBuffers?: false }):
  M & { stats: AdjacencyStats };
export function smoothMesh<M extends MeshBuffers>(device: HipDevice, mesh: M, iterations?: number | null, options?: SmoothOptions & { asBuffers?: false }):
  Omit<M, 'vertices'> & { vertices: Float32Array; stats: AdjacencyStats };
export function smoothMesh(device: HipDevice, mesh: MeshArrays | MeshBuffers, iterations: number | null | undefined, options: SmoothOptions & { asBuffers: true }):
  MeshBuffers & { stats: AdjacencyStats; numVertices: number; numFaces: number };
/** The area-weighted unit normals [V*3] of the mesh; (0, 0, 0) for a vertex without a face of non-zero finite area. */
export function vertexNormals(device: HipDevice, mesh: MeshArrays | MeshBuffers): Float32Array;
/** extractMesh's last stages in their order -- smoothMesh, simplifyMesh from `origin`, vertexNormals -- each only when asked for (null, null, false: none). */
export function finishMesh(device: HipDevice, mesh: MeshArrays | MeshBuffers, origin: ArrayLike<number>, smooth: number | null, simplify: number | null, normals: boolean,
                           read?: (device: HipDevice, mesh: MeshBuffers) => object): any;
/** The face classes of a MeshRasterizer's last encode -- every face is in exactly one -- the pixels some face covers, and whether the camera block was of another
 *  image size (nothing is drawn then). */
export interface RasterStats { invalidFaces: number; clippedFaces: number; degenerateFaces: number; culledFaces: number; emptyFaces: number; rasterizedFaces: number;
                               coveredPixels: number; viewportMismatch: number }
export type CullMode = 'none' | 'back' | 'front';
export type RasterOutput = 'depth' | 'face' | 'colour' | 'normal';
export const CULL_MODES: { none: 0; back: 1; front: 2 };
/** A face whose bounding box exceeds this many pixels on either axis is drawn by the kernel of 8 x 8 blocks (WDGS_MESH_RASTER_LARGE_FACE_PIXELS). */
export const MESH_RASTER_LARGE_FACE_PIXELS: number;
/** The default near depth: the depth below which the forward pass drops a Gaussian. */
export const MESH_RASTER_NEAR: number;
export const NO_FACE: 0xFFFFFFFF;
/** A z-buffered triangle rasterizer under the library's camera block (wdgs_mesh_rasterizer): depth f32, face u32, colour rgba8 and normal rgba32f images of an
 *  indexed mesh on the device, each byte a function of the input alone.  No clipping: a face with a vertex nearer than `near` is dropped.  No reference counterpart. */
export class MeshRasterizer {
  constructor(device: HipDevice);
  encode(vertices: HipBuffer | null, numVertices: number, faces: HipBuffer | null, numFaces: number, colours: HipBuffer | null, camera: HipBuffer, width: number, height: number,
         options?: { near?: number | null; cull?: CullMode; depth?: HipBuffer | null; face?: HipBuffer | null; colour?: HipBuffer | null; normal?: HipBuffer | null }): void;
  stats(): RasterStats;
  destroy(): void;
}
export interface MeshImages { depth?: Float32Array; face?: Uint32Array; colour?: Uint8Array; normal?: Float32Array; stats: RasterStats }
export interface MeshImageBuffers { depth?: HipBuffer; face?: HipBuffer; colour?: HipBuffer; normal?: HipBuffer; stats: RasterStats }
/** The images of `mesh` under `camera` (the 68-float block); options.outputs defaults to ['depth', 'face']; row-major, width x height. */
export function rasterizeMesh(device: HipDevice, mesh: MeshArrays | MeshBuffers, camera: Float32Array | HipBuffer, width: number, height: number,
                              options?: { near?: number | null; cull?: CullMode; outputs?: RasterOutput[]; asBuffers?: false }): MeshImages;
export function rasterizeMesh(device: HipDevice, mesh: MeshArrays | MeshBuffers, camera: Float32Array | HipBuffer, width: number, height: number,
                              options: { near?: number | null; cull?: CullMode; outputs?: RasterOutput[]; asBuffers: true }): MeshImageBuffers;
/** depthAgreement's counts: the pixels where both, a alone, b alone have a depth; those of `both` within the threshold; the quantised sum and the mean of |a - b|. */
export interface DepthAgreement { both: number; onlyA: number; onlyB: number; within: number; sum_q: number; mean: number }
export function encodeDepthAgreement(device: HipDevice, a: HipBuffer, b: HipBuffer, width: number, height: number, maxDifference: number, threshold: number, out: HipBuffer,
                                     options?: { bWeightSum?: HipBuffer | null; minWeightSum?: number }): void;
export function depthAgreementResult(sums: ArrayLike<number | bigint>, maxDifference: number): DepthAgreement;
export function depthAgreement(device: HipDevice, a: Float32Array | HipBuffer, b: Float32Array | HipBuffer, width: number, height: number, maxDifference: number,
                               threshold: number, options?: { bWeightSum?: Float32Array | HipBuffer | null; minWeightSum?: number }): DepthAgreement;
export function meshOnDevice(device: HipDevice, mesh: MeshArrays | MeshBuffers, what: string): { vertices: HipBuffer; faces: HipBuffer; V: number; F: number; own: boolean };
/** The index of "no point found" (PointIndex.nearest).  No reference counterpart. */
export const NO_INDEX: 0xFFFFFFFF;
export interface MeshSamples { points: Float32Array; face: Uint32Array; count: number }
export interface MeshSampleBuffers { points: HipBuffer; face: HipBuffer; count: number }
/** Area-weighted surface sampling of a triangle mesh on the device (wdgs_mesh_sampler): count, then emit with the same arguments.  No reference counterpart. */
export class MeshSampler {
  constructor(device: HipDevice);
  count(vertices: HipBuffer, numVertices: number, faces: HipBuffer, numFaces: number, density: number, seed?: number): number;
  emit(vertices: HipBuffer, numVertices: number, faces: HipBuffer, numFaces: number, density: number, seed: number, points: HipBuffer, face?: HipBuffer | null,
       capacity?: number | null): void;
  destroy(): void;
}
/** Points on the surface of a mesh, `density` per unit area on average; a function of its arguments alone, bit for bit.  No reference counterpart. */
export function sampleMesh(device: HipDevice, mesh: { vertices: Float32Array | HipBuffer; faces: Uint32Array | HipBuffer }, density: number, seed?: number,
                           options?: { asBuffers?: false }): MeshSamples;
export function sampleMesh(device: HipDevice, mesh: { vertices: Float32Array | HipBuffer; faces: Uint32Array | HipBuffer }, density: number, seed: number,
                           options: { asBuffers: true }): MeshSampleBuffers;
export interface MeshComponentLabels { count: number; faceComponent: Uint32Array; vertexComponent: Uint32Array; triangles: Uint32Array; vertices: Uint32Array;
                                       invalidFaces: number }
export interface ComponentSelection { keepLargest?: number | null; minTriangles?: number; minFraction?: number }
export interface CompactedMesh extends TriangleMesh { vertexMap: Uint32Array; faceMap: Uint32Array; components: Uint32Array }
/** Connected components of an indexed mesh on the device (wdgs_mesh_components): label, select, compact.  No reference counterpart. */
export class MeshComponents {
  constructor(device: HipDevice);
  readonly numFaces: number; readonly numVertices: number; readonly count: number; readonly invalidFaces: number;
  label(faces: HipBuffer | null, numFaces: number, numVertices: number): number;
  read(): MeshComponentLabels;
  select(keep: ArrayLike<number | boolean>): { vertices: number; faces: number };
  compact(vertices: HipBuffer | null, verticesOut: HipBuffer | null, facesOut: HipBuffer, vertexMap?: HipBuffer | null, faceMap?: HipBuffer | null,
          capacityVertices?: number | null, capacityFaces?: number | null): void;
  destroy(): void;
}
/** The connected components of a mesh: connectivity through shared vertices, components numbered in ascending order of their lowest vertex; a function of
 *  the mesh alone, bit for bit.  No reference counterpart. */
export function meshComponents(device: HipDevice, mesh: { vertices: Float32Array | HipBuffer; faces: Uint32Array | HipBuffer }): MeshComponentLabels;
/** Which components to keep (Uint8Array[C] of 0 / 1), ranked by (triangles descending, component number ascending).  Host side.  No reference counterpart. */
export function selectComponents(triangles: ArrayLike<number>, options?: ComponentSelection): Uint8Array;
/** The mesh without the components selectComponents does not keep; colours and keys follow vertexMap.  No reference counterpart. */
export function removeSmallComponents(device: HipDevice, mesh: { vertices: Float32Array | HipBuffer; faces: Uint32Array | HipBuffer; colours?: Uint8Array | null;
                                      keys?: BigUint64Array | null }, options?: ComponentSelection): CompactedMesh;
/** The rule on per-face counters: pixels >= minPixels (1), views >= minViews (1), agreeing >= minAgreeing (0) and agreeing 65536 >=
 *  rint(minAgreeingFraction 65536) pixels (0). */
export interface FaceRule { minPixels?: number; minViews?: number; minAgreeing?: number; minAgreeingFraction?: number }
export interface FaceVisibilityStats { views: number; foreignPixels: number; countedPixels: number; agreeingPixels: number }
export interface FilteredMesh { vertices: Float32Array; faces: Uint32Array; vertexMap: Uint32Array; faceMap: Uint32Array; invalidFaces: number;
                                colours?: Uint8Array | null; keys?: BigUint64Array | null }
export interface FilteredMeshBuffers { vertices: HipBuffer; faces: HipBuffer; vertexMap: HipBuffer; faceMap: HipBuffer; numVertices: number; numFaces: number;
                                       invalidFaces: number }
/** Per-face counters over views (wdgs_face_visibility): u32[F][3] = { pixels, agreeing, views }, integer sums of the rasterizer's face images.  No reference
 *  counterpart. */
export class FaceVisibility {
  constructor(device: HipDevice);
  readonly numFaces: number;
  reset(numFaces: number): void;
  accumulate(faceImage: HipBuffer | null, width: number, height: number, options?: { meshDepth?: HipBuffer | null; modelDepth?: HipBuffer | null;
             modelWeightSum?: HipBuffer | null; minWeightSum?: number; threshold?: number }): void;
  buffer(): HipBuffer | null;
  read(): Uint32Array;
  flags(keep: HipBuffer | null, rule?: FaceRule): void;
  stats(): FaceVisibilityStats;
  destroy(): void;
}
/** keep u8[numFaces] from counters u32[numFaces][3], both on the device, by the rule.  Stream-ordered.  No reference counterpart. */
export function encodeFaceVisibilityFlags(device: HipDevice, counters: HipBuffer | null, numFaces: number, keep: HipBuffer | null, rule?: FaceRule): void;
/** Which faces to keep (Uint8Array[F] of 0 / 1) from counters Uint32Array[3 F]: the host restatement of FaceVisibility.flags.  No reference counterpart. */
export function selectFaces(counters: ArrayLike<number>, rule?: FaceRule): Uint8Array;
/** MeshComponents' compaction for an arbitrary face mask (wdgs_mesh_face_filter): select, compact.  No reference counterpart. */
export class MeshFaceFilter {
  constructor(device: HipDevice);
  select(faces: HipBuffer | null, numFaces: number, numVertices: number, keep: HipBuffer | null): { vertices: number; faces: number; invalidFaces: number };
  compact(vertices: HipBuffer | null, verticesOut: HipBuffer | null, facesOut: HipBuffer | null, vertexMap?: HipBuffer | null, faceMap?: HipBuffer | null,
          capacityVertices?: number | null, capacityFaces?: number | null): void;
  destroy(): void;
}
/** The mesh without the faces whose flag is zero and the vertices no kept face names; colours and keys follow vertexMap.  No reference counterpart. */
export function filterFaces(device: HipDevice, mesh: MeshArrays | MeshBuffers, keep: ArrayLike<number | boolean> | HipBuffer, options?: { asBuffers?: false }): FilteredMesh;
export function filterFaces(device: HipDevice, mesh: MeshArrays | MeshBuffers, keep: ArrayLike<number | boolean> | HipBuffer, options: { asBuffers: true }): FilteredMeshBuffers;
/** Which faces of a mesh the cameras see, without a model: every camera's face image rasterized and accumulated.  No reference counterpart. */
export function faceVisibility(device: HipDevice, mesh: MeshArrays | MeshBuffers, cameras: Array<Float32Array | HipBuffer>, width: number, height: number,
                               options?: { near?: number; cull?: 'none' | 'back' | 'front' }): { counters: Uint32Array; stats: FaceVisibilityStats };
export interface BakeStats { usable: number; inImage: number; visible: number; accumulated: number; viewportMismatch: number; bakedVertices: number }
/** bakeVertexColours' options: normals (true: the mesh's normals, or vertexNormals' when it carries none, weigh the views; false: every view weighs the
 *  same), depthTolerance (0.05), minCos (0.1: a caller's knob, not a tuned number), minViews (1), minWeight (1), near, occlusion (true), asBuffers. */
export interface BakeOptions { normals?: boolean; depthTolerance?: number; minCos?: number; minViews?: number; minWeight?: number | bigint; near?: number;
                               occlusion?: boolean; asBuffers?: boolean }
export interface BakeView { camera: HipBuffer; image: HipBuffer; width: number; height: number }
/** Per-vertex colour sums over views (wdgs_mesh_colour_baker): u64[V][4] = { R, G, B, Wt } and u32[V] views, integer sums of bilinear samples of the
 *  photographs weighted by the cosine to the camera.  No reference counterpart. */
export class MeshColourBaker {
  constructor(device: HipDevice);
  readonly numVertices: number;
  reset(numVertices: number): void;
  accumulate(vertices: HipBuffer | null, numVertices: number, camera: HipBuffer | null, image: HipBuffer | null, width: number, height: number,
             options?: { normals?: HipBuffer | null; meshDepth?: HipBuffer | null; near?: number; depthTolerance?: number; minCos?: number }): void;
  resolve(coloursOut: HipBuffer | null, numVertices: number, options?: { fallback?: HipBuffer | null; bakedOut?: HipBuffer | null; minViews?: number;
          minWeight?: number | bigint }): void;
  read(): { sums: BigUint64Array; views: Uint32Array };
  stats(): BakeStats;
  destroy(): void;
}
/** The mesh with colours: Uint8Array[3 V] taken from the photographs, baked: Uint8Array[V] and stats; with asBuffers colours rgba8[V] and baked u8[V] stay on
 *  the device.  No reference counterpart. */
export function bakeVertexColours(device: HipDevice, mesh: MeshArrays | MeshBuffers, cameras: Array<Float32Array | HipBuffer>, images: Array<Uint8Array | HipBuffer>,
                                  width: number, height: number, options?: BakeOptions): BakedMesh;
/** bakeVertexColours for views on the device, which may differ in size. */
export function bakeMeshFromViews(device: HipDevice, mesh: MeshArrays | MeshBuffers, views: BakeView[], options?: BakeOptions, what?: string): BakedMesh;
export type BakedMesh = { [key: string]: unknown; colours: Uint8Array | HipBuffer; baked: Uint8Array | HipBuffer; stats: BakeStats };
export interface TextureStats { invalidFaces: number; facingAwayFaces: number; offImageFaces: number; usable: number; inImage: number; visible: number; accumulated: number;
                                viewportMismatch: number; bakedTexels: number; filledTexels: number; fallbackTexels: number }
/** bakeTexture's options: cell (8: the edge of the square cell two faces share, 4, 8, 16 or 32 texels), depthTolerance (0.05), minCos (0.1), minWeight (1),
 *  near, occlusion (true), twoSided (false), fill (true: an unseen texel next to seen ones of its face takes their mean), asBuffers. */
export interface TextureOptions { cell?: number; depthTolerance?: number; minCos?: number; minWeight?: number; near?: number; occlusion?: boolean; twoSided?: boolean;
                                  fill?: boolean; asBuffers?: boolean }
export interface TextureLayout { width: number; height: number; cellsPerRow: number }
/** The atlas of numFaces faces in cells of `cell` texels and its per-corner texture coordinates uv: Float32Array[F * 6] (OBJ convention).  Arithmetic alone. */
export function textureLayout(numFaces: number, cell?: number): TextureLayout & { uv: Float32Array };
/** Per-texel colour sums of a mesh's texture atlas over views (wdgs_mesh_texture_baker): u32[cells cell cell][4] = { R, G, B, Wsum }, cell-major.  No reference
 *  counterpart. */
export class MeshTextureBaker {
  constructor(device: HipDevice);
  readonly numFaces: number;
  readonly cell: number;
  readonly width: number;
  readonly height: number;
  readonly cellsPerRow: number;
  reset(numFaces: number, cell?: number, accumulates?: number): TextureLayout;
  accumulate(vertices: HipBuffer | null, numVertices: number, faces: HipBuffer | null, numFaces: number, camera: HipBuffer | null, image: HipBuffer | null, width: number,
             height: number, options?: { meshDepth?: HipBuffer | null; near?: number; depthTolerance?: number; minCos?: number; twoSided?: boolean }): void;
  resolve(faces: HipBuffer | null, numFaces: number, numVertices: number, textureOut: HipBuffer | null,
          options?: { colours?: HipBuffer | null; stateOut?: HipBuffer | null; minWeight?: number; fill?: boolean }): void;
  read(): Uint32Array;
  stats(): TextureStats;
  destroy(): void;
}
/** The mesh with texture: Uint8Array[Ht Wt 4], uv: Float32Array[F * 6], texelState: Uint8Array[Ht Wt], textureWidth, textureHeight, textureCell and textureStats;
 *  with asBuffers texture and texelState stay on the device.  No reference counterpart. */
export function bakeTexture(device: HipDevice, mesh: MeshArrays | MeshBuffers, cameras: Array<Float32Array | HipBuffer>, images: Array<Uint8Array | HipBuffer>,
                            width: number, height: number, options?: TextureOptions): TexturedMesh;
/** bakeTexture for views on the device, which may differ in size. */
export function bakeTextureFromViews(device: HipDevice, mesh: MeshArrays | MeshBuffers, views: BakeView[], options?: TextureOptions, what?: string): TexturedMesh;
export type TexturedMesh = { [key: string]: unknown; texture: Uint8Array | HipBuffer; uv: Float32Array; texelState: Uint8Array | HipBuffer; textureWidth: number;
                             textureHeight: number; textureCell: number; textureStats: TextureStats };
/** colours and keys of a typed-array mesh gathered through out.vertexMap into out. */
export function gatherVertexAttributes(mesh: { colours?: unknown; keys?: unknown }, out: { vertexMap: Uint32Array; colours?: Uint8Array | null; keys?: BigUint64Array | null }): void;
/** A uniform grid over points for exact nearest-point queries under a cutoff (wdgs_point_index); the cell edge is a speed parameter only.  No reference
 *  counterpart. */
export class PointIndex {
  constructor(device: HipDevice, points: Float32Array | HipBuffer, options?: { cellSize?: number | null; count?: number | null });
  readonly numPoints: number;
  info(): { cellSize: number; dims: number[]; indexed: number };
  reserveQueries(count: number): void;
  nearestInto(encoder: HipEncoder | null, queries: HipBuffer, count: number, maxDistance: number, d2: HipBuffer, index: HipBuffer, pairs?: HipBuffer | null): void;
  nearest(queries: Float32Array | HipBuffer, maxDistance: number): { d2: Float32Array; index: Uint32Array };
  /** The bounding box of the finite points. */
  bounds(): { lo: Float32Array; hi: Float32Array };
  /** The k (1 to 16) nearest within maxDistance by (squared distance, index) into rows of d2 f32[count][k] and index u32[count][k], padded with +inf and
   *  NO_INDEX; excludeSelf: query i leaves out the indexed point i.  Stream-ordered; records. */
  kNearestInto(encoder: HipEncoder | null, queries: HipBuffer, count: number, k: number, maxDistance: number, d2: HipBuffer, index: HipBuffer,
               excludeSelf?: boolean, pairs?: HipBuffer | null): void;
  kNearest(queries: Float32Array | HipBuffer, k: number, maxDistance: number, excludeSelf?: boolean): { d2: Float32Array; index: Uint32Array };
  destroy(): void;
}
/** wdgs_point_index_k_nearest's flag bit 0.  No reference counterpart. */
export const KNN_EXCLUDE_SELF: 1;
/** 3DGS's scale initialisation from the k nearest neighbours, written in place into pointCloud.gaussian_3d_buffer (DESIGN.md section 15).  No reference
 *  counterpart. */
export function initScalesFromNeighbours(device: HipDevice, pointCloud: PointCloud,
                                         options?: { k?: number; maxDistance?: number | null; minD2?: number; count?: number | null }): { meanD2: Float32Array; found: Uint32Array };
export interface PointDistanceStats { n: number; n_found: number; n_within: number; sum_q: number; mean: number }
/** Stream-ordered pointDistanceStats: three u64 { n_found, n_within, sum_q } into the first 24 bytes of `out`. */
export function encodePointDistanceStats(device: HipDevice, d2: HipBuffer, count: number, maxDistance: number, threshold: number, out: HipBuffer): void;
export function pointDistanceStats(device: HipDevice, d2: Float32Array | HipBuffer, maxDistance: number, threshold: number, count?: number | null): PointDistanceStats;
export interface GeometryMetrics {
  accuracy: number; completeness: number; chamfer: number; precision: number; recall: number; fscore: number;
  n_points: number; n_reference: number; outliers_points: number; outliers_reference: number;
}
/** Accuracy, completeness, Chamfer distance and precision / recall / F-score of a point set against a reference set.  No reference counterpart. */
export function geometryMetrics(device: HipDevice, points: Float32Array | HipBuffer, reference: Float32Array | HipBuffer, maxDistance: number, threshold: number,
                                options?: { numPoints?: number | null; numReference?: number | null }): GeometryMetrics;
/** The packed word of a Gaussian without a normal.  No reference counterpart. */
export const NO_NORMAL: 0x80008000;
export interface NormalAgreement { sum_e: number; sum_a: number; pixels: number; value: number }
/** The normals of an f32 depth image (central differences of its back-projection): rgba32f { n, 1 }, zero where a neighbour is missing.  `camera`: the
 *  68-float block or [proj[0][0], proj[1][1]].  No reference counterpart. */
export function depthToNormals(device: HipDevice, depth: HipBuffer, width: number, height: number, camera: ArrayLike<number>, target: HipBuffer): void;
/** Stream-ordered normalAgreement: three u64 { sum e, sum a, pixels } into the first 24 bytes of `out`. */
export function encodeNormalAgreement(device: HipDevice, normal: HipBuffer, depthNormals: HipBuffer, width: number, height: number, out: HipBuffer): void;
/** The weight-averaged 1 - cos between a composited normal image and a depth-normal image, with its exact integer sums (synchronises).  No reference counterpart. */
export function normalAgreement(device: HipDevice, normal: HipBuffer, depthNormals: HipBuffer, width: number, height: number): NormalAgreement;
/** A normal image as rgba8 for presentation (facing the camera: blue; no normal: black).  No reference counterpart. */
export function normalToRGBA8(device: HipDevice, normal: HipBuffer, width: number, height: number, target: HipBuffer): void;
/** The C-ABI communicator (wdgs_comm_*): RCCL on the device's stream, for the data-parallel step of a host without torch.distributed. */
export class Communicator {
  constructor(device: HipDevice, uniqueId: ArrayBuffer, worldSize: number, rank: number);
  readonly worldSize: number; readonly rank: number;
  static uniqueId(): ArrayBuffer;
  exchangeGradients(grad: HipBuffer, visible: HipBuffer, flag: HipBuffer | null, slicePoints: number): void;
  allgatherRows(rows: HipBuffer, slicePoints: number): void;
  broadcast(ptr: bigint, bytes: number, root: number): void;
  allreduceCounts(counts: HipBuffer, count: number): void;
  allreduceGradients(grad: HipBuffer, visible: HipBuffer, numPoints: number): void;
  static groupStart(): void; static groupEnd(): void;
  destroy(): void;
}
