// Typings of evaluation.js: the evaluation side of a Trainer (no reference counterpart).  The Trainer's methods of the same names delegate here; their
// typings in trainer.d.ts carry the descriptions.
import { ComponentSelection, CompactedMesh, ContributionRecords, GeometryMetrics, HipBuffer, SimplifiedMesh, TriangleMesh, TSDFVolume } from './webdgs_hip';
import { CameraData } from './loaders';
import { LoadedImage } from './images';
import { EvaluationResult, NormalConsistencyResult, Trainer, TrainingImage, TrainingView } from './trainer';

type Split = 'eval' | 'train';
type DepthKind = 'median' | 'expected';
type MeshOptions = { viewIds?: number[] | null; split?: Split; depthKind?: DepthKind; minWeight?: number; truncation?: number; maxWeight?: number; colour?: boolean; weld?: 'host' | 'device'; simplify?: number | null; smooth?: number | null; normals?: boolean; cull?: import('./trainer').CullMeshOptions | null; bake?: boolean | import('./trainer').BakeMeshOptions | null; texture?: boolean | import('./trainer').TextureMeshOptions | null } & ComponentSelection;

export class Evaluator {
  /** Uses of the trainer only: device, pointCloud, iteration, trainCameras, images, cameraBuffers, newPassSet, dcWords, longLists, drain(), growTileEntryCapacity(). */
  constructor(trainer: Trainer);
  readonly trainer: Trainer;
  readonly cameras: TrainingView[]; readonly images: TrainingImage[];
  /** Tile-entry lists of the evaluation passes (0: what the training passes get); Trainer.evalMaxTileEntries reads and writes it. */
  maxTileEntries: number;
  setEvaluationViews(cameras: (TrainingView | CameraData)[], images: (TrainingImage | LoadedImage)[]): void;
  evaluate(viewIds?: number[] | null, split?: Split): EvaluationResult;
  normalConsistency(viewIds?: number[] | null, split?: Split, depthKind?: DepthKind): NormalConsistencyResult;
  meshDepthAgreement(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: import('./trainer').MeshDepthAgreementOptions):
    import('./trainer').MeshDepthAgreementResult;
  meshVisibility(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: import('./trainer').MeshVisibilityOptions):
    import('./trainer').MeshVisibilityResult;
  cullMesh(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: import('./trainer').CullMeshOptions):
    import('./webdgs_hip').FilteredMesh & { counters: Uint32Array; views: number[] };
  bakeMeshColours(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: import('./trainer').BakeMeshOptions):
    import('./webdgs_hip').BakedMesh & { views: number[] };
  bakeMeshTexture(mesh: import('./webdgs_hip').MeshArrays | import('./webdgs_hip').MeshBuffers, options?: import('./trainer').TextureMeshOptions):
    import('./webdgs_hip').TexturedMesh & { views: number[] };
  fuseDepth(volume: TSDFVolume, viewIds?: number[] | null, split?: Split, depthKind?: DepthKind): number[];
  extractMesh(lo: ArrayLike<number>, hi: ArrayLike<number>, voxelSize: number, options?: MeshOptions): TriangleMesh | CompactedMesh | SimplifiedMesh | import('./webdgs_hip').FilteredMesh | import('./webdgs_hip').BakedMesh;
  evaluateGeometry(reference: Float32Array | string, lo: ArrayLike<number>, hi: ArrayLike<number>, voxelSize: number, maxDistance: number, threshold: number,
                   options?: { density?: number | null; seed?: number } & MeshOptions): GeometryMetrics & { vertices: number; faces: number; samples: number; ms: number };
  contributionStats(viewIds?: number[] | null, split?: Split): ContributionRecords & { views: number[] };
  /** The views' contribution records accumulated into one new device buffer, which the caller destroys (Trainer.pruneByContribution decides on it). */
  contributionBuffer(viewIds: number[] | null | undefined, split: Split, what: string): { stats: HipBuffer; ids: number[] };
  destroy(): void;
}
