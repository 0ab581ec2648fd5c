// node bindings/napi/tsdf_run.js <dir> -- TSDF fusion and mesh extraction through the node host (tests/test_gpu_tsdf_napi.py): the synthetic scene of
// meta.json (bindings/ts/synth.js generates the very bits webdgs_amd/synth.py does) from meta.cameras cameras of a circle; each view's median depth,
// weight sum and colour are fused into a TSDFVolume, whose arrays, triangle buffers and welded mesh (as a PLY) go back as raw files; then
// Trainer.fuseDepth over meta.train_views into a second volume.
'use strict';
const fs = require('fs');
const path = require('path');
const ts = (m) => require(path.join(__dirname, '..', 'ts', m));
const hip = ts('webdgs_hip.js'), synth = ts('synth.js'), loaders = ts('loaders.js');
const { Trainer } = ts('trainer.js');

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));

function main() {
  const cfg = meta.config, px = cfg.width * cfg.height;
  const dev = new hip.HipDevice(0);
  const scene = synth.makeGaussians(cfg), cams = synth.circleCameras(cfg, meta.cameras);
  const upload = (words) => { const b = dev.createBuffer({ size: words.byteLength }); dev.queue.writeBuffer(b, 0, words); return b; };
  const pc = { type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) };
  const cbuf = upload(cams[0]);
  const fwd = new hip.TiledForwardPass(dev, pc, cbuf, { viewportWidth: cfg.width, viewportHeight: cfg.height, renderMode: 'gaussian' });
  const rast = new hip.TiledRasterizer({ device: dev, forwardPass: fwd, format: 'rgba8unorm' });
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const vol = new hip.TSDFVolume(dev, meta.origin, meta.voxel_size, meta.dims);
  refused('emit before count', 'WDGS_E_STATE', () => hip.addon.tsdfVolumeEmitTriangles(vol.handle, cbuf.ptr, null, null, 0));
  for (const cam of cams) {
    dev.queue.writeBuffer(cbuf, 0, cam);
    fwd.encode(null);
    rast.encode(null, cfg.width, cfg.height);
    rast.encodeDepth(null, ['median', 'weight_sum']);
    vol.integrate(rast.getDepthTextureView('median'), cbuf, cfg.width, cfg.height, { weightSum: rast.getDepthTextureView('weight_sum'), colour: rast.getOutputTextureView() });
  }
  refused('integrate with the wrong image size', 'WDGS_E_STATE', () => vol.integrate(rast.getDepthTextureView('median'), cbuf, cfg.height, cfg.width));
  const n = vol.numVoxels;
  fs.writeFileSync(path.join(dir, 'out_tsdf.f32'), Buffer.from(dev.readBuffer(vol.getTSDFBuffer(), 4 * n)));
  fs.writeFileSync(path.join(dir, 'out_weight.f32'), Buffer.from(dev.readBuffer(vol.getWeightBuffer(), 4 * n)));
  fs.writeFileSync(path.join(dir, 'out_rgb.f32'), Buffer.from(dev.readBuffer(vol.getColourBuffer(), 12 * n)));
  const tri = vol.extractTriangles();
  const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
  fs.writeFileSync(path.join(dir, 'out_positions.f32'), raw(tri.positions));
  fs.writeFileSync(path.join(dir, 'out_keys.u64'), raw(tri.keys));
  fs.writeFileSync(path.join(dir, 'out_colours.rgba'), raw(tri.colours));
  const mesh = vol.extractMesh();
  loaders.saveMeshPLY(path.join(dir, 'out_mesh.ply'), mesh);
  const plain = new hip.TSDFVolume(dev, meta.origin, meta.voxel_size, [4, 3, 2], { colour: false });
  refused('colour to a volume without colour', 'WDGS_E_STATE', () => plain.integrate(rast.getDepthTextureView('median'), cbuf, cfg.width, cfg.height, { colour: rast.getOutputTextureView() }));
  const emptyCount = plain.countTriangles();
  plain.destroy();

  // the trainer: fuseDepth over the training views before any step (the images are never looked at: blank)
  const view = (v) => ({ camera: cams[v], width: cfg.width, height: cfg.height });
  const blank = () => { const b = dev.createBuffer({ size: 4 * px }); hip.addon.bufferClear(dev.handle, b.ptr, b.size); return { texture: b, width: cfg.width, height: cfg.height }; };
  const t = new Trainer(dev, undefined, {});
  t.setDensifyPruneConfig({ schedule: { enabled: false } });
  t.setPointCloud({ type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) });
  t.setDataset(meta.train_views.map(view), meta.train_views.map(blank));
  t.start();
  const tvol = new hip.TSDFVolume(dev, meta.origin, meta.voxel_size, meta.dims);
  const fused = t.fuseDepth(tvol, meta.fuse_order);
  fs.writeFileSync(path.join(dir, 'out_trainer_tsdf.f32'), Buffer.from(dev.readBuffer(tvol.getTSDFBuffer(), 4 * n)));
  fs.writeFileSync(path.join(dir, 'out_trainer_rgb.f32'), Buffer.from(dev.readBuffer(tvol.getColourBuffer(), 12 * n)));
  const lo = meta.origin, hi = meta.origin.map((o, a) => o + meta.dims[a] * meta.voxel_size * 0.999);
  const tmesh = t.extractMesh(lo, hi, meta.voxel_size, { viewIds: meta.fuse_order });
  tvol.destroy();
  t.destroy();
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify({ errors, triangles: tri.count, vertices: mesh.vertices.length / 3, empty_count: emptyCount, fused,
    trainer_mesh_faces: tmesh.faces.length / 3, dims: hip.addon.tsdfVolumeGetDims(vol.handle), truncation: vol.truncation }));
  vol.destroy(); rast.destroy(); fwd.destroy(); cbuf.destroy();
  pc.gaussian_3d_buffer.destroy(); pc.sh_buffer.destroy();
  dev.destroy();
  console.log('TSDF_RUN_OK');
}

main();
