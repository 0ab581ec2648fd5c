// node bindings/napi/normal_run.js <dir> -- the normal maps through the node host (tests/test_gpu_normal_napi.py): the synthetic scene of meta.json
// (bindings/ts/synth.js generates the very bits webdgs_amd/synth.py does) at one camera of a circle; TiledRasterizer.encodeNormal writes the packed words
// and the composited image, depthToNormals the normals of the median depth, normalAgreement the three sums, normalToRGBA8 the presentation bytes,
// Viewer.renderNormals the image again through the viewer's own passes, Trainer.normalConsistency the sums per view.  Everything goes back as raw files.
'use strict';
const fs = require('fs');
const path = require('path');
const ts = (m) => require(path.join(__dirname, '..', 'ts', m));
const hip = ts('webdgs_hip.js'), synth = ts('synth.js');
const { Viewer } = ts('viewer.js');
const { Trainer } = ts('trainer.js');

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));

function main() {
  const cfg = meta.config, px = cfg.width * cfg.height;
  const dev = new hip.HipDevice(0);
  const scene = synth.makeGaussians(cfg), cam = synth.circleCameras(cfg, meta.cameras)[meta.view];
  const upload = (words) => { const b = dev.createBuffer({ size: words.byteLength }); dev.queue.writeBuffer(b, 0, words); return b; };
  const pc = { type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) };
  const cbuf = upload(cam);
  const fwd = new hip.TiledForwardPass(dev, pc, cbuf, { viewportWidth: cfg.width, viewportHeight: cfg.height, renderMode: 'gaussian' });
  const rast = new hip.TiledRasterizer({ device: dev, forwardPass: fwd, format: 'rgba8unorm' });
  const errors = [];
  const refused = (what, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== 'WDGS_E_STATE') errors.push(`${what}: ${e.code || e}`); } };
  refused('encodeNormal before encode', () => rast.encodeNormal(null));
  fwd.encode(null);
  rast.encode(null, cfg.width, cfg.height);
  refused('getNormalTextureView before encodeNormal', () => rast.getNormalTextureView());
  refused('getGaussianNormals before encodeNormal', () => rast.getGaussianNormals());
  rast.encodeNormal(null);
  rast.encodeDepth(null, ['median']);
  fs.writeFileSync(path.join(dir, 'out_words.u32'), Buffer.from(dev.readBuffer(rast.getGaussianNormals(), 4 * cfg.num_points)));
  fs.writeFileSync(path.join(dir, 'out_normal.f32'), Buffer.from(dev.readBuffer(rast.getNormalTextureView(), 16 * px)));
  const dn = dev.createBuffer({ size: 16 * px }), rgba = dev.createBuffer({ size: 4 * px });
  hip.depthToNormals(dev, rast.getDepthTextureView('median'), cfg.width, cfg.height, cam, dn);
  fs.writeFileSync(path.join(dir, 'out_depth_normals.f32'), Buffer.from(dev.readBuffer(dn, 16 * px)));
  const agreement = hip.normalAgreement(dev, rast.getNormalTextureView(), dn, cfg.width, cfg.height);
  hip.normalToRGBA8(dev, rast.getNormalTextureView(), cfg.width, cfg.height, rgba);
  fs.writeFileSync(path.join(dir, 'out_rgba.rgba'), Buffer.from(dev.readBuffer(rgba, 4 * px)));

  // the viewer: starts in point-cloud mode; the camera block goes straight into its uniform buffer
  const viewer = new Viewer(dev, null, { width: cfg.width, height: cfg.height }, 'rgba8unorm');
  viewer.setPointCloud(pc);
  dev.queue.writeBuffer(viewer.camera.uniform_buffer, 0, cam);
  viewer.render(null);
  const before = Buffer.from(viewer.readFrame().buffer);
  fs.writeFileSync(path.join(dir, 'out_viewer_normal.f32'), Buffer.from(viewer.renderNormals().buffer));
  viewer.saveNormalPNG(path.join(dir, 'out_viewer_normal.png'));
  viewer.render(null);
  const after = Buffer.from(viewer.readFrame().buffer);

  // the trainer: meta.train_views cameras of the circle to train on, meta.eval_views to hold out (the images are never looked at: blank);
  // normalConsistency before any step, per view and for both depth kinds
  const cams = synth.circleCameras(cfg, meta.cameras);
  const view = (v) => ({ camera: cams[v], width: cfg.width, height: cfg.height });
  const blank = () => { const b = dev.createBuffer({ size: 4 * px }); hip.addon.bufferClear(dev.handle, b.ptr, b.size); return { texture: b, width: cfg.width, height: cfg.height }; };
  const t = new Trainer(dev, undefined, {});
  t.setDensifyPruneConfig({ schedule: { enabled: false } });
  t.setPointCloud({ type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) });
  t.setDataset(meta.train_views.map(view), meta.train_views.map(blank));
  t.setEvaluationViews(meta.eval_views.map(view), meta.eval_views.map(blank));
  t.start();
  const pick = (r) => ({ views: r.views, sum_e: r.sum_e, sum_a: r.sum_a, pixels: r.pixels, value: r.value, mean: r.mean, iteration: r.iteration });
  const consistency = { eval_median: pick(t.normalConsistency()), train_expected: pick(t.normalConsistency([1, 0], 'train', 'expected')) };
  try { t.normalConsistency([99]); errors.push('normalConsistency of a view that is not there: not refused'); } catch (e) { if (!(e instanceof RangeError)) errors.push(`normalConsistency([99]): ${e}`); }
  t.destroy();
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify({ errors, agreement, consistency, no_normal: hip.NO_NORMAL, render_mode: viewer.settings.renderMode,
    frame_unchanged: before.equals(after) }));
  viewer.destroy(); dn.destroy(); rgba.destroy(); rast.destroy(); fwd.destroy(); cbuf.destroy();
  pc.gaussian_3d_buffer.destroy(); pc.sh_buffer.destroy();
  dev.destroy();
  console.log('NORMAL_RUN_OK');
}

main();
