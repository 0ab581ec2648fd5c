// node bindings/napi/meshvisibility_run.js <dir> -- per-face visibility, its rule and the face filter through the node host
// (tests/test_gpu_meshvisibility_napi.py): every image of meta.images (<name>.face.u32 and, with depth, <name>.a.f32, <name>.b.f32, <name>.ws.f32, raw
// little-endian) is accumulated twice into one FaceVisibility, with and without its depth images; every rule of meta.rules is applied to counters.u32 on the
// device and on the host; mesh.vertices.f32 / mesh.faces.u32 go through filterFaces under every mask of meta.masks (<name>.keep.u8); the sphere of
// sphere.vertices.f32 / sphere.faces.u32 goes through faceVisibility under sphere.cameras.f32 and is culled.  With meta.trainer (a cloud, a dataset and a mesh:
// gaussians.bin, sh.bin, cameras.bin, images.bin, fused.vertices.f32, fused.faces.u32) a Trainer runs meshVisibility and cullMesh.  SHA-256 digests of the
// outputs go to out.json and are printed.
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
// one digest over a mesh's arrays in a fixed order (tests/test_gpu_meshvisibility_napi.py: mesh_digest)
const meshDigest = (m) => sha(m.vertices, m.faces, m.vertexMap, m.faceMap);

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 16) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };

  // 1. the crafted images: two views each on one object, with the depth images and without
  const images = {};
  const visibility = new hip.FaceVisibility(dev);
  refused('accumulate before reset', 'WDGS_E_STATE', () => visibility.accumulate(null, 1, 1));
  for (const c of meta.images) {
    const bufs = { face: upload(readAs(`${c.name}.face.u32`, Uint32Array)), a: upload(readAs(`${c.name}.a.f32`, Float32Array)), b: upload(readAs(`${c.name}.b.f32`, Float32Array)),
      ws: upload(readAs(`${c.name}.ws.f32`, Float32Array)) };
    visibility.reset(c.faces);
    visibility.accumulate(bufs.face, c.width, c.height, { meshDepth: bufs.a, modelDepth: bufs.b, modelWeightSum: bufs.ws, minWeightSum: c.min_weight_sum, threshold: c.threshold });
    visibility.accumulate(bufs.face, c.width, c.height);
    images[c.name] = { counters: sha(visibility.read()), stats: visibility.stats() };
    dev.synchronize();
    hip.destroyBuffers(bufs);
  }
  // refusals
  const image = dev.createBuffer({ size: 64 });
  visibility.reset(3);
  refused('a width of zero', 'WDGS_E', () => visibility.accumulate(image, 0, 4));
  refused('a threshold of zero', 'WDGS_E', () => visibility.accumulate(image, 4, 4, { threshold: 0 }));
  refused('one depth image', 'WDGS_E', () => visibility.accumulate(image, 4, 4, { meshDepth: image }));
  refused('a null face image', 'WDGS_E', () => visibility.accumulate(null, 4, 4));
  for (let k = 0; k < 63; k++) visibility.accumulate(image, 1, 1);
  refused('a view that could overflow', 'WDGS_E_CAPACITY', () => visibility.accumulate(null, 8192, 8192));
  refused('a fraction above one', 'WDGS_E', () => hip.selectFaces(new Uint32Array(3), { minAgreeingFraction: 1.5 }));
  visibility.destroy();
  image.destroy();

  // 2. the rule, on the device and on the host
  const counters = readAs('counters.u32', Uint32Array), F = counters.length / 3;
  const cbuf = upload(counters), keep = dev.createBuffer({ size: Math.max(F, 16) });
  const rules = meta.rules.map((rule) => {
    hip.encodeFaceVisibilityFlags(dev, cbuf, F, keep, rule);
    return { device: sha(new Uint8Array(dev.readBuffer(keep, F))), host: sha(hip.selectFaces(counters, rule)) };
  });
  cbuf.destroy(); keep.destroy();

  // 3. the filter under every mask: typed arrays, then device buffers left on the device
  const mesh = { vertices: readAs('mesh.vertices.f32', Float32Array), faces: readAs('mesh.faces.u32', Uint32Array) };
  const masks = {};
  for (const name of meta.masks) {
    const k = readAs(`${name}.keep.u8`, Uint8Array);
    const host = hip.filterFaces(dev, mesh, k);
    const src = { vertices: upload(mesh.vertices), faces: upload(mesh.faces), numVertices: mesh.vertices.length / 3, numFaces: mesh.faces.length / 3 }, kbuf = upload(k);
    const b = hip.filterFaces(dev, src, kbuf, { asBuffers: true });
    const bytes = (buf, n) => (n ? dev.readBuffer(buf, n) : new ArrayBuffer(0));
    const device = { vertices: new Float32Array(bytes(b.vertices, 12 * b.numVertices)), faces: new Uint32Array(bytes(b.faces, 12 * b.numFaces)),
      vertexMap: new Uint32Array(bytes(b.vertexMap, 4 * b.numVertices)), faceMap: new Uint32Array(bytes(b.faceMap, 4 * b.numFaces)) };
    masks[name] = { host: meshDigest(host), device: meshDigest(device), vertices: host.vertexMap.length, faces: host.faceMap.length, invalidFaces: host.invalidFaces };
    hip.destroyBuffers(b); hip.destroyBuffers(src); kbuf.destroy();
  }
  const filt = new hip.MeshFaceFilter(dev);
  refused('compact before select', 'WDGS_E_STATE', () => filt.compact(null, null, null));
  filt.destroy();

  // 4. the sphere under its cameras, culled
  const ball = { vertices: readAs('sphere.vertices.f32', Float32Array), faces: readAs('sphere.faces.u32', Uint32Array) };
  const cams = readAs('sphere.cameras.f32', Float32Array), cameras = [];
  for (let v = 0; v * 68 < cams.length; v++) cameras.push(cams.slice(68 * v, 68 * v + 68));
  const seen = hip.faceVisibility(dev, ball, cameras, meta.sphere.width, meta.sphere.height, { near: meta.sphere.near });
  const culled = hip.filterFaces(dev, ball, hip.selectFaces(seen.counters));
  const sphere = { counters: sha(seen.counters), stats: seen.stats, culled: meshDigest(culled), faces: culled.faceMap.length };

  // 5. meshVisibility and cullMesh through the Trainer
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
    const fused = { vertices: readAs('fused.vertices.f32', Float32Array), faces: readAs('fused.faces.u32', Uint32Array) };
    const r = t.meshVisibility(fused, { threshold: m.threshold });
    const c = t.cullMesh(fused, Object.assign({ threshold: m.threshold }, m.rule));
    trainer = { views: r.views, counters: sha(r.counters), counted: r.counted, agreeing: r.agreeing, foreign: r.foreign, iteration: r.iteration, culled: meshDigest(c),
      culledCounters: sha(c.counters), faces: c.faceMap.length };
    t.destroy();
  }

  const out = { errors, images, rules, masks, sphere, trainer };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHVISIBILITY_RUN_OK');
}

main();
