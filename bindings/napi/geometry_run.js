// node bindings/napi/geometry_run.js <dir> -- the mesh accuracy metrics through the node host (tests/test_gpu_geometry_napi.py): the mesh, point set and
// queries of <dir> (raw little-endian files) go through sampleMesh, PointIndex.nearest, pointDistanceStats and geometryMetrics, whose outputs go back as raw
// files, the samples also as a points PLY; then Trainer.evaluateGeometry on the synthetic scene of meta.json (bindings/ts/synth.js generates the very bits
// webdgs_amd/synth.py does) against the reference PLY of <dir>, before any step.
'use strict';
const fs = require('fs');
const path = require('path');
const ts = (m) => require(path.join(__dirname, '..', 'ts', m));
const hip = ts('webdgs_hip.js'), synth = ts('synth.js'), loaders = ts('loaders.js');
const { Trainer } = ts('trainer.js');

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const raw = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (words) => { const b = dev.createBuffer({ size: Math.max(words.byteLength, 4) }); if (words.byteLength) dev.queue.writeBuffer(b, 0, words); return b; };

  // 1. sampling
  const mesh = { vertices: readAs('mesh_vertices.f32', Float32Array), faces: readAs('mesh_faces.u32', Uint32Array) };
  const samples = hip.sampleMesh(dev, mesh, meta.density, meta.seed);
  fs.writeFileSync(path.join(dir, 'out_samples.f32'), raw(samples.points));
  fs.writeFileSync(path.join(dir, 'out_face.u32'), raw(samples.face));
  loaders.savePointsPLY(path.join(dir, 'out_samples.ply'), samples.points);
  const back = loaders.loadPointsPLY(path.join(dir, 'out_samples.ply'));
  if (Buffer.compare(raw(back), raw(samples.points)) !== 0) errors.push('the points PLY does not read back exactly');
  const vb = upload(mesh.vertices), fb = upload(mesh.faces), room = dev.createBuffer({ size: 12 * Math.max(samples.count, 1) });
  const sampler = new hip.MeshSampler(dev);
  refused('emit before count', 'WDGS_E_STATE', () => sampler.emit(vb, mesh.vertices.length / 3, fb, mesh.faces.length / 3, meta.density, meta.seed, room));
  const counted = sampler.count(vb, mesh.vertices.length / 3, fb, mesh.faces.length / 3, meta.density, meta.seed);
  refused('emit with too little room', 'WDGS_E_CAPACITY', () => sampler.emit(vb, mesh.vertices.length / 3, fb, mesh.faces.length / 3, meta.density, meta.seed, room, null, counted - 1));
  sampler.destroy(); vb.destroy(); fb.destroy(); room.destroy();

  // 2. nearest points, 3. the sums, and the metrics
  const points = readAs('points.f32', Float32Array), queries = readAs('queries.f32', Float32Array);
  const index = new hip.PointIndex(dev, points, { cellSize: meta.cell_size });
  const near = index.nearest(queries, meta.cutoff);
  refused('a cutoff of 0', 'WDGS_E', () => index.nearest(queries, 0));
  const info = index.info();
  index.destroy();
  fs.writeFileSync(path.join(dir, 'out_d2.f32'), raw(near.d2));
  fs.writeFileSync(path.join(dir, 'out_index.u32'), raw(near.index));
  const stats = hip.pointDistanceStats(dev, near.d2, meta.cutoff, meta.threshold);
  const metrics = hip.geometryMetrics(dev, queries, points, meta.cutoff, meta.threshold);

  // 4. the trainer: evaluateGeometry over the training views before any step (the images are never looked at: blank)
  const cfg = meta.config, px = cfg.width * cfg.height;
  const scene = synth.makeGaussians(cfg), cams = synth.circleCameras(cfg, meta.cameras);
  const view = (v) => ({ camera: cams[v], width: cfg.width, height: cfg.height });
  const blank = () => { const b = dev.createBuffer({ size: 4 * px }); hip.addon.bufferClear(dev.handle, b.ptr, b.size); return { texture: b, width: cfg.width, height: cfg.height }; };
  const t = new Trainer(dev, undefined, {});
  t.setDensifyPruneConfig({ schedule: { enabled: false } });
  t.setPointCloud({ type: 'full', num_points: cfg.num_points, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(scene.gaussians), sh_buffer: upload(scene.sh) });
  t.setDataset(meta.train_views.map(view), meta.train_views.map(blank));
  t.start();
  const evaluated = t.evaluateGeometry(path.join(dir, 'reference.ply'), meta.lo, meta.hi, meta.voxel_size, meta.eval_max_distance, meta.eval_threshold,
    { viewIds: meta.fuse_order, seed: meta.seed });
  t.destroy();
  delete evaluated.ms;
  const nanToNull = (o) => Object.fromEntries(Object.entries(o).map(([k, v]) => [k, Number.isNaN(v) ? 'nan' : v]));
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify({ errors, samples: samples.count, info, stats: nanToNull(stats), metrics: nanToNull(metrics),
    evaluated: nanToNull(evaluated) }));
  dev.destroy();
  console.log('GEOMETRY_RUN_OK');
}

main();
