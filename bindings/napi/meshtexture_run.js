// node bindings/napi/meshtexture_run.js <dir> -- a texture atlas baked from photographs through the node host (tests/test_gpu_meshtexture_napi.py): every case
// of meta.cases (<name>.vertices.f32, <name>.faces.u32, <name>.colours.u8 and per view <name>.<k>.camera.f32, <name>.<k>.image.u8, <name>.<k>.depth.f32, raw
// little-endian; what meta says is absent is not there) is accumulated view by view into one MeshTextureBaker and resolved; the sphere of sphere.vertices.f32 /
// sphere.faces.u32 / sphere.colours.u8 goes through bakeTexture under sphere.cameras.f32 and sphere.images.u8, with and without occlusion.  With meta.trainer (a cloud, a dataset and a mesh: gaussians.bin, sh.bin, cameras.bin, images.bin, fused.vertices.f32, fused.faces.u32,
// fused.colours.u8) a Trainer runs bakeMeshTexture.  SHA-256 digests of
// the outputs and of textureLayout's coordinates go to out.json and are printed.
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
const STATS = ['invalidFaces', 'facingAwayFaces', 'offImageFaces', 'usable', 'inImage', 'visible', 'accumulated', 'viewportMismatch', 'bakedTexels', 'filledTexels',
  'fallbackTexels'];
const statWords = (stats) => BigUint64Array.from(STATS, (k) => BigInt(stats[k]));

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 16) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };

  // 1. the crafted cases: one digest over rows, texture, texel states and the totals (tests/meshtexture_ref.py: digest), one over the layout's coordinates
  const cases = {}, layouts = {};
  const baker = new hip.MeshTextureBaker(dev);
  const one = dev.createBuffer({ size: 272 });
  refused('accumulate before reset', 'WDGS_E_STATE', () => baker.accumulate(null, 0, null, 0, one, one, 1, 1));
  refused('resolve before reset', 'WDGS_E_STATE', () => baker.resolve(null, 0, 0, null));
  for (const c of meta.cases) {
    const V = c.vertices, F = c.faces, bufs = { vertices: upload(readAs(`${c.name}.vertices.f32`, Float32Array)), faces: upload(readAs(`${c.name}.faces.u32`, Uint32Array)) };
    if (c.colours) bufs.colours = upload(readAs(`${c.name}.colours.u8`, Uint8Array));
    const L = baker.reset(F, c.cell), n = L.width * L.height, host = hip.textureLayout(F, c.cell);
    if (host.width !== L.width || host.height !== L.height || host.cellsPerRow !== L.cellsPerRow) errors.push(`${c.name}: textureLayout and the library disagree`);
    layouts[c.name] = sha(host.uv);
    bufs.texture = dev.createBuffer({ size: Math.max(4 * n, 16) });
    bufs.state = dev.createBuffer({ size: Math.max(n, 16) });
    c.views.forEach((w, k) => {
      const v = { camera: upload(readAs(`${c.name}.${k}.camera.f32`, Float32Array)), image: upload(readAs(`${c.name}.${k}.image.u8`, Uint8Array)) };
      if (w.depth) v.depth = upload(readAs(`${c.name}.${k}.depth.f32`, Float32Array));
      baker.accumulate(bufs.vertices, V, bufs.faces, F, v.camera, v.image, w.width, w.height, { meshDepth: v.depth || null, near: w.near, depthTolerance: w.depth_tolerance,
        minCos: w.min_cos, twoSided: w.two_sided });
      dev.synchronize();
      hip.destroyBuffers(v);
    });
    baker.resolve(bufs.faces, F, V, bufs.texture, { colours: bufs.colours || null, stateOut: bufs.state, minWeight: c.min_weight, fill: c.fill });
    const bytes = (b, k) => new Uint8Array(k ? dev.readBuffer(b, k) : new ArrayBuffer(0));
    cases[c.name] = sha(baker.read(), bytes(bufs.texture, 4 * n), bytes(bufs.state, n), statWords(baker.stats()));
    hip.destroyBuffers(bufs);
  }
  // refusals
  const some = dev.createBuffer({ size: 64 });
  refused('a cell of five texels', 'WDGS_E', () => baker.reset(3, 5));
  baker.reset(3, 8);
  refused('a width of zero', 'WDGS_E', () => baker.accumulate(some, 3, some, 3, one, some, 0, 2));
  refused('a negative tolerance', 'WDGS_E', () => baker.accumulate(some, 3, some, 3, one, some, 2, 2, { depthTolerance: -1 }));
  refused('a cosine above one', 'WDGS_E', () => baker.accumulate(some, 3, some, 3, one, some, 2, 2, { minCos: 1.5 }));
  refused('a null image', 'WDGS_E', () => baker.accumulate(some, 3, some, 3, one, null, 2, 2));
  refused('another face count', 'WDGS_E_STATE', () => baker.accumulate(some, 3, some, 2, one, some, 2, 2));
  refused('a negative minWeight', 'WDGS_E', () => baker.resolve(some, 3, 3, some, { minWeight: -1 }));
  baker.reset(3, 8, 65535);
  refused('the 65536th view', 'WDGS_E_STATE', () => baker.accumulate(some, 3, some, 3, one, some, 2, 2));
  baker.destroy();
  some.destroy();
  one.destroy();

  // 2. the sphere under its cameras, with and without occlusion
  const ball = { vertices: readAs('sphere.vertices.f32', Float32Array), faces: readAs('sphere.faces.u32', Uint32Array), colours: readAs('sphere.colours.u8', Uint8Array) };
  const s = meta.sphere, cams = readAs('sphere.cameras.f32', Float32Array), photos = readAs('sphere.images.u8', Uint8Array), cameras = [], images = [];
  for (let v = 0; v * 68 < cams.length; v++) {
    cameras.push(cams.slice(68 * v, 68 * v + 68));
    images.push(photos.slice(4 * s.width * s.height * v, 4 * s.width * s.height * (v + 1)));
  }
  const sphere = {};
  for (const occlusion of [true, false]) {
    const r = hip.bakeTexture(dev, ball, cameras, images, s.width, s.height, { cell: s.cell, depthTolerance: s.depth_tolerance, minCos: s.min_cos, near: s.near, occlusion });
    sphere[occlusion ? 'occlusion' : 'plain'] = { texture: sha(r.texture), state: sha(r.texelState), uv: sha(r.uv), size: [r.textureWidth, r.textureHeight], stats: r.textureStats };
    if (occlusion) {   // the OBJ, its MTL and its PNG: the test compares the three files with the Python host's, byte for byte, and what loadMeshOBJ gives back
      const loaders = require(path.join(__dirname, '..', 'ts', 'loaders.js')), file = path.join(dir, 'js', 'mesh.obj');
      fs.mkdirSync(path.join(dir, 'js'), { recursive: true });
      loaders.saveMeshOBJ(file, r);
      const back = loaders.loadMeshOBJ(file);
      for (const k of ['vertices', 'faces', 'uv', 'texture']) if (sha(back[k]) !== sha(r[k])) errors.push(`loadMeshOBJ: ${k} differs from what was saved`);
      if (back.textureWidth !== r.textureWidth || back.textureHeight !== r.textureHeight || back.normals !== undefined) errors.push('loadMeshOBJ: the texture size or the keys differ');
    }
  }

  // 3. bakeMeshTexture and extractMesh's option through the Trainer
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
    const r = t.bakeMeshTexture(fused, { depthTolerance: m.depth_tolerance, cell: 4 });
    const few = t.bakeMeshTexture(fused, { depthTolerance: m.depth_tolerance, viewIds: [2], occlusion: false, fill: false });
    const ex = t.extractMesh(m.lo, m.hi, m.voxel, { texture: { depthTolerance: m.depth_tolerance, cell: 4 } });
    const extracted = { vertices: sha(ex.vertices), faces: sha(ex.faces), texture: sha(ex.texture), uv: sha(ex.uv), stats: ex.textureStats, views: ex.views };
    trainer = { views: r.views, texture: sha(r.texture), state: sha(r.texelState), stats: r.textureStats, fewViews: few.views, fewTexture: sha(few.texture), fewStats: few.textureStats, extracted };
    t.destroy();
  }

  const out = { errors, cases, layouts, sphere, trainer };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHTEXTURE_RUN_OK');
}

main();
