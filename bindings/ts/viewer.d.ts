// Typings of viewer.js: src/viewer.ts without the browser.
import { DepthKind, HipBuffer, HipDevice, HipEncoder, PointCloud, RenderMode, TiledForwardPass } from './webdgs_hip';
import { Camera, CanvasLike } from './camera';
export type FrameTarget = HipBuffer & { width: number; height: number };
export class Viewer {
  constructor(device: HipDevice, context: { getCurrentTexture(): FrameTarget } | null, canvas: CanvasLike, format: string);
  readonly camera: Camera; readonly cameraControl: { update(dt: number): void };
  setPointCloud(pointCloud: PointCloud): void;
  update(dt: number): void;
  render(commandEncoder: HipEncoder | null): void;
  setRenderMode(mode: RenderMode): void;
  setGaussianScale(value: number): void;
  setPointSize(value: number): void;
  getForwardPass(): TiledForwardPass | null;
  currentTexture(): FrameTarget;
  resize(width: number, height: number): void;
  readFrame(): Uint8Array;
  /** The current camera's depth image (width * height f32), rendered in gaussian mode; the render mode is left as it was.  No reference counterpart. */
  renderDepth(kind?: DepthKind): Float32Array;
  /** The current camera's normal map (width * height * 4 f32: N.x, N.y, N.z, A), rendered in gaussian mode; the render mode is left as it was.  No reference counterpart. */
  renderNormals(): Float32Array;
  /** The normal map as a colour PNG (facing the camera: blue).  No reference counterpart. */
  saveNormalPNG(file: string): void;
  savePNG(file: string): void;
  destroy(): void;
}
