// node bindings/napi/meshbake_run.js <dir> -- vertex colours baked from photographs through the node host (tests/test_gpu_meshbake_napi.py): every case of
// meta.cases (<name>.vertices.f32, <name>.normals.f32, <name>.fallback.u8 and per view <name>.<k>.camera.f32, <name>.<k>.image.u8, <name>.<k>.depth.f32, raw
// little-endian; what meta says is absent is not there) is accumulated view by view into one MeshColourBaker and resolved; the sphere of sphere.vertices.f32 /
// sphere.faces.u32 / sphere.colours.u8 / sphere.normals.f32 goes through bakeVertexColours under sphere.cameras.f32 and sphere.images.u8, with and without
// occlusion.  With meta.trainer (a cloud, a dataset and a mesh: gaussians.bin, sh.bin, cameras.bin, images.bin, fused.vertices.f32, fused.faces.u32,
// fused.colours.u8) a Trainer runs bakeMeshColours.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const sha = (...arrays) => {
  const h = crypto.createHash('sha256');
  for (const a of arrays) h.update(Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  return h.digest('hex');
};
const STATS = ['usable', 'inImage', 'visible', 'accumulated', 'viewportMismatch', 'bakedVertices'];
const statWords = (stats) => BigUint64Array.from(STATS, (k) => BigInt(stats[k]));

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 16) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };

  // 1. the crafted cases: one digest over sums, views, colours, the mask and the totals (tests/meshbake_ref.py: digest)
  const cases = {};
  const baker = new hip.MeshColourBaker(dev);
  const one = dev.createBuffer({ size: 272 });
  refused('accumulate before reset', 'WDGS_E_STATE', () => baker.accumulate(null, 0, one, one, 1, 1));
  refused('resolve before reset', 'WDGS_E_STATE', () => baker.resolve(null, 0));
  for (const c of meta.cases) {
    const V = c.vertices, bufs = { vertices: upload(readAs(`${c.name}.vertices.f32`, Float32Array)) };
    if (c.normals) bufs.normals = upload(readAs(`${c.name}.normals.f32`, Float32Array));
    if (c.fallback) bufs.fallback = upload(readAs(`${c.name}.fallback.u8`, Uint8Array));
    bufs.colours = dev.createBuffer({ size: Math.max(4 * V, 16) });
    bufs.baked = dev.createBuffer({ size: Math.max(V, 16) });
    baker.reset(V);
    c.views.forEach((w, k) => {
      const v = { camera: upload(readAs(`${c.name}.${k}.camera.f32`, Float32Array)), image: upload(readAs(`${c.name}.${k}.image.u8`, Uint8Array)) };
      if (w.depth) v.depth = upload(readAs(`${c.name}.${k}.depth.f32`, Float32Array));
      baker.accumulate(bufs.vertices, V, v.camera, v.image, w.width, w.height, { normals: bufs.normals || null, meshDepth: v.depth || null, near: w.near,
        depthTolerance: w.depth_tolerance, minCos: w.min_cos });
      dev.synchronize();
      hip.destroyBuffers(v);
    });
    baker.resolve(bufs.colours, V, { fallback: bufs.fallback || null, bakedOut: bufs.baked, minViews: c.min_views, minWeight: c.min_weight });
    const state = baker.read(), bytes = (b, n) => new Uint8Array(n ? dev.readBuffer(b, n) : new ArrayBuffer(0));
    cases[c.name] = sha(state.sums, state.views, bytes(bufs.colours, 4 * V), bytes(bufs.baked, V), statWords(baker.stats()));
    hip.destroyBuffers(bufs);
  }
  // refusals
  baker.reset(3);
  const some = dev.createBuffer({ size: 64 });
  refused('a width of zero', 'WDGS_E', () => baker.accumulate(some, 3, one, some, 0, 2));
  refused('a negative tolerance', 'WDGS_E', () => baker.accumulate(some, 3, one, some, 2, 2, { depthTolerance: -1 }));
  refused('a cosine above one', 'WDGS_E', () => baker.accumulate(some, 3, one, some, 2, 2, { minCos: 1.5 }));
  refused('a null image', 'WDGS_E', () => baker.accumulate(some, 3, one, null, 2, 2));
  refused('another vertex count', 'WDGS_E_STATE', () => baker.accumulate(some, 2, one, some, 2, 2));
  refused('a negative minViews', 'WDGS_E', () => baker.resolve(some, 3, { minViews: -1 }));
  baker.destroy();
  some.destroy();
  one.destroy();

  // 2. the sphere under its cameras, with and without occlusion
  const ball = { vertices: readAs('sphere.vertices.f32', Float32Array), faces: readAs('sphere.faces.u32', Uint32Array), colours: readAs('sphere.colours.u8', Uint8Array),
    normals: readAs('sphere.normals.f32', Float32Array) };
  const s = meta.sphere, cams = readAs('sphere.cameras.f32', Float32Array), photos = readAs('sphere.images.u8', Uint8Array), cameras = [], images = [];
  for (let v = 0; v * 68 < cams.length; v++) {
    cameras.push(cams.slice(68 * v, 68 * v + 68));
    images.push(photos.slice(4 * s.width * s.height * v, 4 * s.width * s.height * (v + 1)));
  }
  const sphere = {};
  for (const occlusion of [true, false]) {
    const r = hip.bakeVertexColours(dev, ball, cameras, images, s.width, s.height, { depthTolerance: s.depth_tolerance, minCos: s.min_cos, near: s.near, occlusion });
    sphere[occlusion ? 'occlusion' : 'plain'] = { colours: sha(r.colours), baked: sha(r.baked), stats: r.stats };
  }

  // 3. bakeMeshColours through the Trainer
  let trainer = null;
  if (meta.trainer) {
    const { Trainer } = require(path.join(__dirname, '..', 'ts', 'trainer.js'));
    const m = meta.trainer, u8 = (name) => readAs(name, Uint8Array);
    const pc = { type: 'full', num_points: m.num_points, sh_deg: m.sh_deg, gaussian_3d_buffer: upload(u8('gaussians.bin')), sh_buffer: upload(u8('sh.bin')) };
    const blocks = readAs('cameras.bin', Float32Array), imgBytes = u8('images.bin');
    const views = [], targets = [];
    let at = 0;
    m.sizes.forEach(([w, h], v) => {
      views.push({ camera: blocks.slice(v * 68, v * 68 + 68), width: w, height: h });
      targets.push({ texture: upload(imgBytes.subarray(at, at + 4 * w * h)), width: w, height: h });
      at += 4 * w * h;
    });
    const t = new Trainer(dev);
    t.setDensifyPruneConfig({ schedule: { enabled: false } });
    t.setPointCloud(pc);
    t.setDataset(views, targets);
    t.start();
    const fused = { vertices: readAs('fused.vertices.f32', Float32Array), faces: readAs('fused.faces.u32', Uint32Array), colours: u8('fused.colours.u8') };
    const r = t.bakeMeshColours(fused, { depthTolerance: m.depth_tolerance });
    const few = t.bakeMeshColours(fused, { depthTolerance: m.depth_tolerance, viewIds: [2], normals: false, occlusion: false });
    trainer = { views: r.views, colours: sha(r.colours), baked: sha(r.baked), stats: r.stats, fewViews: few.views, fewColours: sha(few.colours), fewStats: few.stats };
    t.destroy();
  }

  const out = { errors, cases, sphere, trainer };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHBAKE_RUN_OK');
}

main();
