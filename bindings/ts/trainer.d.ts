// Typings of trainer.js: the public surface of the reference's Trainer (src/trainer.ts:177-566).
import { AdamHyperparameters, ContributionRecords, HipBuffer, HipDevice, OptimizerInitialState, PointCloud, TrainingConfig } from './webdgs_hip';
import { CameraData } from './loaders';
import { LoadedImage } from './images';
import { Exchange } from './parallel';
import { Evaluator } from './evaluation';

export interface DensifyPruneTrainingConfig {   // trainer.ts:23-40
  schedule: { enabled: boolean; warmupIterations: number; interval: number; stopIterations: number };
  metricViews: number; metricDownscale: number; metricThreshold: number; maxBufferBytes: number; maxNewPointsPerStep: number;
  pruneOpacity: number; cloneThresholdCount: number; splitScaleThreshold: number;
}
export interface TrainingView { camera: Float32Array; width: number; height: number; }   // the 68-float CameraUniforms block of the view
export interface TrainingImage { texture: HipBuffer; width: number; height: number; }    // rgba8, row-major (LoadedImage.texture)
export interface PointCloudSwapRequest { pointCloud: PointCloud; optimizerInitialState?: OptimizerInitialState; }

export interface TrainerOptions {
  random?: () => number; useCommandBuffers?: boolean; maxTileEntries?: number; reusePasses?: boolean; deferredSH?: boolean;
  /** the single-view step runs K17 + Adam + re-pack as one kernel (default true); keepGradients also fills backwardPass.getGradientsBuffer() */
  fuseGeometryAdam?: boolean; keepGradients?: boolean;
  /** 1: every step awaits its own completion (trainer.ts:639-645); 2..4: a step awaits the one pipelineDepth - 1 submissions ago */
  pipelineDepth?: number;
  /** views per rank per global step (a batched step: BASELINE config c4), device lanes they are dealt to (default 3), view-batched K1 / K17 (default on) */
  viewsPerStep?: number; lanes?: number; batchViews?: boolean;
  /** device lanes the metric views of a densify event are dealt to (default 3; integer counts: any order gives the same bits) */
  metricLanes?: number;
  /** view-sharded data parallelism (parallel.js) */
  worldSize?: number; rank?: number; exchange?: Exchange;
}
export class Trainer {
  constructor(device: HipDevice, trainingConfig?: TrainingConfig, options?: TrainerOptions);
  /** Deferred SH writes: brings pointCloud.sh_buffer up to date for a device-side reader of the raw rows (host reads and forward passes built on the cloud follow by themselves). */
  flushPointCloud(): void;
  /** step() on a given global batch of views (worldSize * viewsPerStep indices); no reference counterpart. */
  stepViews(viewIds?: number[]): Promise<void>;
  /** maxTileEntries for a new forward pass: the caller's, or what an overflow has grown the library-sized lists to (0 = the library's sizing). */
  tileEntries(): number;
  /** Doubles the library-sized tile-entry lists after a WDGS_E_CAPACITY report and rebuilds the passes; false when the caller pinned maxTileEntries. */
  growTileEntryCapacity(error: Error): boolean;
  /** device.queue.wait / device.synchronize through CapacityReports.settle: a report about this trainer's passes is thrown, other owners' lines are left for them. */
  wait(ticket: number): void;
  synchronize(): void;
  /** Records every view's command buffers up front; the number of steps taken depends on the dataset size only. */
  warmupCommandBuffers(): Promise<number>;
  /** Awaits every step still in flight (pipelineDepth > 1). */
  drain(): void;
  /** Data parallelism: every owner broadcasts its slice of the optimizer state (before a densify rebuild, an export). */
  syncOptimizerState(): void;
  pipelineDepth: number; keepGradients: boolean; fuseGeometryAdam: boolean; useCommandBuffers: boolean;
  /** Long tile lists (csrc/longlist.h): null = the library's defaults; set before the first step to give the passes this trainer builds other sizes. */
  longLists: { threshold?: number; maxItems?: number; maxRows?: number; maxItemsCap?: number; maxRowsCap?: number } | null;
  /** Enlarges the long-list scratch of every pass when the last frame wanted more than there is room for (called at densify events). */
  growLongLists(): void;
  readonly lanes: number; readonly viewsPerRank: number; readonly worldSize: number; readonly rank: number;
  random: () => number;
  setPointCloud(pointCloud: PointCloud): void;
  requestPointCloudSwap(pointCloud: PointCloud, optimizerInitialState?: OptimizerInitialState): void;
  consumePointCloudSwapRequest(): PointCloudSwapRequest | null;
  requestResizeTo(numPoints: number): void;
  applyPointCloudSwap(request: PointCloudSwapRequest): void;
  setDataset(cameras: (TrainingView | CameraData)[], images: (TrainingImage | LoadedImage)[]): void;
  /** Views to evaluate on and never to train on (loaders.holdoutSplit); same shapes as setDataset, any image size. */
  setEvaluationViews(cameras: (TrainingView | CameraData)[], images: (TrainingImage | LoadedImage)[]): void;
  /** PSNR (exact SSE kernel) and SSIM (imageSSIM) of the current model on the evaluation views ('eval') or training views ('train'); drains the
   *  pipeline, leaves the training trajectory untouched. */
  evaluate(viewIds?: number[] | null, split?: 'eval' | 'train'): EvaluationResult;
  /** Agreement of the composited normals with the normals of the model's own depth map, per view and weight-averaged over all (1 - cos: a surface
   *  scores near 0); rendered through evaluate's passes, training untouched.  No reference counterpart. */
  normalConsistency(viewIds?: number[] | null, split?: 'eval' | 'train', depthKind?: 'median' | 'expected'): NormalConsistencyResult;
  /** A mesh rasterized under each view against the model's own depth map of that view: per-view and summed counts of the pixels where both, the mesh alone
   *  (onlyA) and the model alone (onlyB: a hole in the mesh) have a depth, and the mean absolute difference; training untouched.  No reference counterpart. */
  meshDepthAgreement(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: MeshDepthAgreementOptions): MeshDepthAgreementResult;
  /** Which faces of a mesh the views see: per face the pixels that show it over all views, those of them where the model's depth map agrees with the mesh's
   *  depth, and the views that show it; per view the pixels counted, agreeing and foreign.  Training untouched.  No reference counterpart. */
  meshVisibility(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: MeshVisibilityOptions): MeshVisibilityResult;
  /** The mesh without the faces the views do not see: meshVisibility's counters, selectFaces' rule and filterFaces, flags and compaction on the device; its
   *  object carries the input's counters and the views.  Training untouched.  No reference counterpart. */
  cullMesh(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: CullMeshOptions):
    import('./webdgs_hip').FilteredMesh & { counters: Uint32Array; views: number[] };
  /** The mesh with its vertex colours taken from the split's photographs under the split's cameras (bakeVertexColours over the trainer's own device copies):
   *  colours, baked and stats replaced or added, and the views.  Training untouched.  No reference counterpart. */
  bakeMeshColours(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: BakeMeshOptions): import('./webdgs_hip').BakedMesh & { views: number[] };
  /** The mesh with a texture atlas taken from the split's photographs under the split's cameras (bakeTexture over the trainer's own device copies): texture,
   *  uv, texelState, textureStats and the atlas's sizes added, and the views.  Training untouched.  No reference counterpart. */
  bakeMeshTexture(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: TextureMeshOptions): import('./webdgs_hip').TexturedMesh & { views: number[] };
  /** Fuses the current model's depth maps (and the rendered colour) into a TSDFVolume, view by view in the order given; rendered through evaluate's
   *  passes, training untouched.  Returns the view list.  No reference counterpart. */
  fuseDepth(volume: import('./webdgs_hip').TSDFVolume, viewIds?: number[] | null, split?: 'eval' | 'train', depthKind?: 'median' | 'expected'): number[];
  /** TSDFVolume.fromBounds -> fuseDepth -> extractMesh -> destroy: the current model as a triangle mesh of the box [lo, hi]; with keepLargest, minTriangles or
   *  minFraction set, without the components removeSmallComponents drops.  weld: 'host' (default) or 'device' -- welded, and with a component rule cleaned,
   *  on the device; the same bytes.  simplify: a cell size -- the mesh is simplified last, by vertex clustering on that grid from lo (simplifyMesh), and
   *  its object is returned.  cull: cullMesh's options -- the faces no view sees are removed after welding and component removal and before smooth, simplify
   *  and normals.  bake: true or bakeMeshColours' options -- the final mesh's colours are taken from the photographs, last.  No reference counterpart. */
  extractMesh(lo: ArrayLike<number>, hi: ArrayLike<number>, voxelSize: number,
              options?: { viewIds?: number[] | null; split?: 'eval' | 'train'; depthKind?: 'median' | 'expected'; minWeight?: number; truncation?: number; maxWeight?: number;
                          colour?: boolean; weld?: 'host' | 'device'; simplify?: number | null; smooth?: number | null; normals?: boolean; cull?: CullMeshOptions | null; bake?: boolean | BakeMeshOptions | null; texture?: boolean | TextureMeshOptions | null } & import('./webdgs_hip').ComponentSelection):
    import('./webdgs_hip').TriangleMesh | import('./webdgs_hip').CompactedMesh | import('./webdgs_hip').SimplifiedMesh | import('./webdgs_hip').FilteredMesh | import('./webdgs_hip').BakedMesh;
  /** extractMesh -> sampleMesh -> geometryMetrics against `reference` (points [M*3], or the path of a PLY): the mesh's accuracy, completeness, Chamfer
   *  distance, precision, recall and F-score, with the mesh's vertex, face and sample counts and ms.  Training untouched.  No reference counterpart. */
  evaluateGeometry(reference: Float32Array | string, lo: ArrayLike<number>, hi: ArrayLike<number>, voxelSize: number, maxDistance: number, threshold: number,
                   options?: { density?: number | null; seed?: number; viewIds?: number[] | null; split?: 'eval' | 'train'; depthKind?: 'median' | 'expected';
                               minWeight?: number; truncation?: number; maxWeight?: number; colour?: boolean; weld?: 'host' | 'device'; simplify?: number | null; smooth?: number | null; normals?: boolean; cull?: CullMeshOptions | null; bake?: boolean | BakeMeshOptions | null; texture?: boolean | TextureMeshOptions | null } &
                     import('./webdgs_hip').ComponentSelection):
    import('./webdgs_hip').GeometryMetrics & { vertices: number; faces: number; samples: number; ms: number };
  /** Per-Gaussian render contribution accumulated over the views (default: all training views); no reference counterpart. */
  contributionStats(viewIds?: number[] | null, split?: 'eval' | 'train'): ContributionRecords & { views: number[] };
  /** Contribution-based pruning: kept iff every criterion given is met; fraction f prunes the Gaussians below the k-th smallest sum_q, k = floor(f N). */
  pruneByContribution(options: { minMaxWeight?: number; minWeightSum?: number; minPixels?: number; fraction?: number; viewIds?: number[] | null }): { before: number; after: number; pruned: number };
  /** Tile-entry lists of the Evaluator's passes (0: what the training passes get); an overflowing view grows them and is rendered again. */
  evalMaxTileEntries: number;
  /** The evaluation side (evaluation.js): the methods from setEvaluationViews to contributionStats above delegate to it. */
  readonly evaluator: Evaluator;
  readonly evalCameras: TrainingView[]; readonly evalImages: TrainingImage[];
  getTrainingConfig(): TrainingConfig; setTrainingConfig(next: Partial<TrainingConfig>): void;
  getOptimizerHyperparameters(): AdamHyperparameters; setOptimizerHyperparameters(next: Partial<AdamHyperparameters>): void;
  setDensifyPruneConfig(next: Partial<DensifyPruneTrainingConfig>): void;
  start(): void; stop(): void; getIsTraining(): boolean;
  setMaxIterations(n: number): void; getMaxIterations(): number;
  getIteration(): number; getPointCount(): number; getLastStepMs(): number; getItersPerSec(): number;
  getLastDensifyPruneIteration(): number | null; getNextDensifyPruneIteration(): number | null;
  step(): Promise<void>;
  destroy(): void;
}
export interface EvaluationResult {
  iteration: number; views: number[]; psnr: number[]; ssim: number[]; sse: number[]; mean_psnr: number; mean_ssim: number; ms: number;
}
export interface MeshDepthAgreementOptions {
  viewIds?: number[] | null; split?: 'eval' | 'train'; depthKind?: 'median' | 'expected'; maxDifference?: number; threshold?: number; minWeightSum?: number;
  near?: number; cull?: 'none' | 'back' | 'front';
}
export interface MeshDepthAgreementResult {
  iteration: number; views: number[]; both: number[]; onlyA: number[]; onlyB: number[]; within: number[]; sum_q: number[]; mean: number[];
  total: import('./webdgs_hip').DepthAgreement; ms: number;
}
export interface MeshVisibilityOptions {
  viewIds?: number[] | null; split?: 'eval' | 'train'; depthKind?: 'median' | 'expected'; threshold?: number; minWeightSum?: number; near?: number;
  cull?: 'none' | 'back' | 'front';
}
export type CullMeshOptions = MeshVisibilityOptions & import('./webdgs_hip').FaceRule;
export type BakeMeshOptions = { viewIds?: number[] | null; split?: 'eval' | 'train' } & import('./webdgs_hip').BakeOptions;
export type TextureMeshOptions = { viewIds?: number[] | null; split?: 'eval' | 'train' } & import('./webdgs_hip').TextureOptions;
export interface MeshVisibilityResult {
  iteration: number; views: number[]; counters: Uint32Array; counted: number[]; agreeing: number[]; foreign: number[]; ms: number;
}
export interface NormalConsistencyResult {
  iteration: number; views: number[]; value: number[]; pixels: number[]; sum_e: number[]; sum_a: number[]; mean: number; ms: number;
}
export function cameraBlockFor(block: Float32Array, width: number, height: number): Float32Array;
export function mat4Inverse(m: ArrayLike<number>): Float32Array;
export function projectionMatrix(znear: number, zfar: number, fovX: number, fovY: number): Float32Array;
export const DEFAULT_DENSIFY: DensifyPruneTrainingConfig;
