// node bindings/napi/meshraster_run.js <dir> -- the mesh rasterizer and the depth agreement through the node host (tests/test_gpu_meshraster_napi.py): every
// case of meta.json (<name>.vertices.f32, <name>.faces.u32, <name>.colours.u8 where it has colours, <name>.camera.f32, raw little-endian, with its viewport, near
// and cull) goes through one MeshRasterizer on device buffers and through rasterizeMesh on typed arrays; every image pair of meta.agreement goes through
// depthAgreement.  With meta.trainer (a cloud, a dataset and a mesh: gaussians.bin, sh.bin, cameras.bin, images.bin, mesh.vertices.f32, mesh.faces.u32) a Trainer
// scores the mesh against its own depth maps with meshDepthAgreement.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const STATS = ['invalidFaces', 'clippedFaces', 'degenerateFaces', 'culledFaces', 'emptyFaces', 'rasterizedFaces', 'coveredPixels', 'viewportMismatch'];
const OUTPUTS = ['depth', 'face', 'colour', 'normal'];
const TYPES = { depth: Float32Array, face: Uint32Array, colour: Uint8Array, normal: Float32Array }, BYTES = { depth: 4, face: 4, colour: 4, normal: 16 };
// one digest over the images in a fixed order (a missing colour image is skipped), then the statistics as u32 (tests/meshraster_ref.py: digest)
const digest = (r) => {
  const h = crypto.createHash('sha256');
  for (const k of OUTPUTS) if (r[k]) h.update(Buffer.from(r[k].buffer, r[k].byteOffset, r[k].byteLength));
  h.update(Buffer.from(Uint32Array.from(STATS.map((k) => r.stats[k])).buffer));
  return h.digest('hex');
};

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };

  // 1. the crafted cases: one object on device buffers with every image read back, then the one-call form on typed arrays
  const cases = {};
  const rasterizer = new hip.MeshRasterizer(dev);
  refused('stats before encode', 'WDGS_E_STATE', () => rasterizer.stats());
  for (const c of meta.cases) {
    const mesh = { vertices: readAs(`${c.name}.vertices.f32`, Float32Array), faces: readAs(`${c.name}.faces.u32`, Uint32Array),
      colours: c.colours ? readAs(`${c.name}.colours.u8`, Uint8Array) : null };
    const camera = readAs(`${c.name}.camera.f32`, Float32Array);
    const V = mesh.vertices.length / 3, F = mesh.faces.length / 3, w = c.width, h = c.height, outputs = OUTPUTS.filter((k) => k !== 'colour' || c.colours);
    const src = { vertices: upload(mesh.vertices), faces: upload(mesh.faces), colours: mesh.colours ? upload(mesh.colours) : null, camera: upload(camera) };
    const out = {};
    for (const k of outputs) out[k] = dev.createBuffer({ size: Math.max(BYTES[k] * w * h, 8) });
    rasterizer.encode(src.vertices, V, src.faces, F, src.colours, src.camera, w, h, Object.assign({ near: c.near, cull: c.cull }, out));
    const got = { stats: rasterizer.stats() };
    for (const k of outputs) got[k] = new TYPES[k](dev.readBuffer(out[k], BYTES[k] * w * h));
    const one = hip.rasterizeMesh(dev, mesh, camera, w, h, { near: c.near, cull: c.cull, outputs });
    cases[c.name] = { device: digest(got), host: digest(one), stats: got.stats };
    hip.destroyBuffers(out);
    hip.destroyBuffers(src);
  }

  // 2. refusals
  const tri = { vertices: upload(Float32Array.from([0, 0, 1, 1, 0, 1, 0, 1, 1])), faces: upload(Uint32Array.from([0, 1, 2])) };
  const cam = upload(readAs(`${meta.cases[0].name}.camera.f32`, Float32Array)), image = dev.createBuffer({ size: 4 * 64 });
  refused('a near of zero', 'WDGS_E', () => rasterizer.encode(tri.vertices, 3, tri.faces, 1, null, cam, 8, 8, { near: 0, depth: image }));
  refused('a width of zero', 'WDGS_E', () => rasterizer.encode(tri.vertices, 3, tri.faces, 1, null, cam, 0, 8, { depth: image }));
  refused('an unknown cull mode', 'WDGS_E', () => rasterizer.encode(tri.vertices, 3, tri.faces, 1, null, cam, 8, 8, { cull: 'sideways', depth: image }));
  refused('a colour image without colours', 'WDGS_E', () => rasterizer.encode(tri.vertices, 3, tri.faces, 1, null, cam, 8, 8, { colour: image }));
  refused('rasterizeMesh: colour without colours', 'WDGS_E', () => hip.rasterizeMesh(dev, { vertices: new Float32Array(9), faces: Uint32Array.from([0, 1, 2]) },
    new Float32Array(68), 8, 8, { outputs: ['colour'] }));
  rasterizer.destroy();
  hip.destroyBuffers(tri);
  cam.destroy(); image.destroy();

  // 3. depth agreement
  const agreement = {};
  for (const c of meta.agreement) {
    const a = readAs(`${c.name}.a.f32`, Float32Array), b = readAs(`${c.name}.b.f32`, Float32Array), ws = c.weight_sum ? readAs(`${c.name}.ws.f32`, Float32Array) : null;
    const r = hip.depthAgreement(dev, a, b, c.width, c.height, c.max_difference, c.threshold, { bWeightSum: ws, minWeightSum: c.min_weight_sum });
    agreement[c.name] = [r.both, r.onlyA, r.onlyB, r.within, r.sum_q];
  }
  refused('a threshold above the maximum', 'WDGS_E', () => hip.depthAgreement(dev, new Float32Array(4), new Float32Array(4), 2, 2, 0.1, 0.2));

  // 4. a mesh against the model's own depth maps, through the Trainer
  let trainer = null;
  if (meta.trainer) {
    const { Trainer } = require(path.join(__dirname, '..', 'ts', 'trainer.js'));
    const m = meta.trainer, u8 = (name) => readAs(name, Uint8Array);
    const pc = { type: 'full', num_points: m.num_points, sh_deg: m.sh_deg, gaussian_3d_buffer: upload(u8('gaussians.bin')), sh_buffer: upload(u8('sh.bin')) };
    const cams = readAs('cameras.bin', Float32Array), imgBytes = u8('images.bin');
    const cameras = [], images = [];
    let at = 0;
    m.sizes.forEach(([w, h], v) => {
      cameras.push({ camera: cams.slice(v * 68, v * 68 + 68), width: w, height: h });
      images.push({ texture: upload(imgBytes.subarray(at, at + 4 * w * h)), width: w, height: h });
      at += 4 * w * h;
    });
    const t = new Trainer(dev);
    t.setDensifyPruneConfig({ schedule: { enabled: false } });
    t.setPointCloud(pc);
    t.setDataset(cameras, images);
    t.start();
    const mesh = { vertices: readAs('mesh.vertices.f32', Float32Array), faces: readAs('mesh.faces.u32', Uint32Array) };
    const r = t.meshDepthAgreement(mesh, { split: 'train', maxDifference: m.max_difference, threshold: m.threshold });
    const one = t.meshDepthAgreement(mesh, { viewIds: [m.sizes.length - 1], split: 'train', maxDifference: m.max_difference, threshold: m.threshold });
    trainer = { views: r.views, both: r.both, onlyA: r.onlyA, onlyB: r.onlyB, within: r.within, sum_q: r.sum_q, total: r.total, iteration: r.iteration,
      last: [one.both[0], one.onlyA[0], one.onlyB[0], one.within[0], one.sum_q[0]] };
    t.destroy();
  }

  const out = { errors, cases, agreement, trainer };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHRASTER_RUN_OK');
}

main();
