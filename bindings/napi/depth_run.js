// node bindings/napi/depth_run.js <dir> -- the depth images through the node host (tests/test_gpu_depth_napi.py): the synthetic scene of meta.json
// (bindings/ts/synth.js generates the very bits webdgs_amd/synth.py does) at one camera of a circle; TiledRasterizer.encodeDepth writes the three
// images, Viewer.renderDepth the median again through the viewer's own passes, depthToRGBA8 the presentation bytes.  Everything goes back as raw files.
'use strict';
const fs = require('fs');
const path = require('path');
const ts = (m) => require(path.join(__dirname, '..', 'ts', m));
const hip = ts('webdgs_hip.js'), synth = ts('synth.js');
const { Viewer } = ts('viewer.js');

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));

function main() {
  const cfg = meta.config, n = 4 * cfg.width * cfg.height;
  const dev = new hip.HipDevice(0);
  const scene = synth.makeGaussians(cfg), cam = synth.circleCameras(cfg, meta.cameras)[meta.view];
  const upload = (words) => { const b = dev.createBuffer({ size: words.byteLength }); dev.queue.writeBuffer(b, 0, words); return b; };
  const pc = { type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) };
  const cbuf = upload(cam);
  const fwd = new hip.TiledForwardPass(dev, pc, cbuf, { viewportWidth: cfg.width, viewportHeight: cfg.height, renderMode: 'gaussian' });
  const rast = new hip.TiledRasterizer({ device: dev, forwardPass: fwd, format: 'rgba8unorm' });
  const errors = [];
  const refused = (what, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== 'WDGS_E_STATE') errors.push(`${what}: ${e.code || e}`); } };
  refused('encodeDepth before encode', () => rast.encodeDepth(null));
  fwd.encode(null);
  rast.encode(null, cfg.width, cfg.height);
  refused('getDepthTextureView before encodeDepth', () => rast.getDepthTextureView('median'));
  rast.encodeDepth(null, ['expected', 'median', 'weight_sum']);
  for (const k of Object.keys(hip.DEPTH_KINDS)) fs.writeFileSync(path.join(dir, `out_${k}.f32`), Buffer.from(dev.readBuffer(rast.getDepthTextureView(k), n)));
  fs.writeFileSync(path.join(dir, 'out_alpha.f32'), Buffer.from(dev.readBuffer(rast.getAlphaTextureView(), n)));
  const grey = dev.createBuffer({ size: n });
  hip.depthToRGBA8(dev, rast.getDepthTextureView(), cfg.width, cfg.height, meta.near, meta.far, grey);
  fs.writeFileSync(path.join(dir, 'out_grey.rgba'), Buffer.from(dev.readBuffer(grey, n)));

  // the viewer: starts in point-cloud mode; the camera block goes straight into its uniform buffer
  const viewer = new Viewer(dev, null, { width: cfg.width, height: cfg.height }, 'rgba8unorm');
  viewer.setPointCloud(pc);
  dev.queue.writeBuffer(viewer.camera.uniform_buffer, 0, cam);
  viewer.render(null);
  const before = Buffer.from(viewer.readFrame().buffer);
  fs.writeFileSync(path.join(dir, 'out_viewer_median.f32'), Buffer.from(viewer.renderDepth('median').buffer));
  viewer.render(null);
  const after = Buffer.from(viewer.readFrame().buffer);
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify({ errors, render_mode: viewer.settings.renderMode, frame_unchanged: before.equals(after) }));
  viewer.destroy(); grey.destroy(); rast.destroy(); fwd.destroy(); cbuf.destroy();
  pc.gaussian_3d_buffer.destroy(); pc.sh_buffer.destroy();
  dev.destroy();
  console.log('DEPTH_RUN_OK');
}

main();
