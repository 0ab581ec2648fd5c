// node bindings/napi/meshsmooth_run.js <dir> -- mesh adjacency, Taubin smoothing and vertex normals through the node host
// (tests/test_gpu_meshsmooth_napi.py): every mesh of meta.json (<name>.vertices.f32, <name>.faces.u32, raw little-endian, with its smoothing arguments) goes
// through one MeshAdjacency on device buffers and through the one-call forms on typed arrays; the volume of <dir> (two spheres) is written through the
// TSDFVolume getters and extracted with options.smooth, normals and simplify under both welds.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));
const loaders = require(path.join(__dirname, '..', 'ts', 'loaders.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const STATS = ['directedEdges', 'edges', 'boundaryEdges', 'nonManifoldEdges', 'invalidFaces', 'boundaryVertices', 'isolatedVertices', 'maxDegree'];
const sha = (arrays, counts) => {
  const h = crypto.createHash('sha256');
  for (const a of arrays) if (a) h.update(Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  if (counts) h.update(Buffer.from(Uint32Array.from(counts).buffer));
  return h.digest('hex');
};
// one digest over the arrays in a fixed order, then the statistics as u32 (tests/meshsmooth_ref.py: digest)
const digest = (r) => sha([r.rowStart, r.neighbours, r.boundary, r.smoothed, r.normals], STATS.map((k) => r.stats[k]));
// a mesh as extractMesh returns it: its arrays in a fixed order (tests/test_gpu_meshsmooth_napi.py: mesh_digest)
const meshDigest = (m) => sha(['vertices', 'faces', 'colours', 'keys', 'faceMap', 'vertexCluster', 'normals'].map((k) => m[k] || null), Object.values(m.stats || {}));

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };
  const bytes = (b, n) => (n ? dev.readBuffer(b, n) : new ArrayBuffer(0));

  // 1. the crafted meshes: one object on device buffers with every output read back, then the one-call forms on typed arrays
  const meshes = {};
  const adj = new hip.MeshAdjacency(dev);
  for (const c of meta.meshes) {
    const mesh = { vertices: readAs(`${c.name}.vertices.f32`, Float32Array), faces: readAs(`${c.name}.faces.u32`, Uint32Array) };
    const V = mesh.vertices.length / 3, F = mesh.faces.length / 3, opt = { lambda: c.lam, mu: c.mu, pinBoundary: c.pin_boundary };
    const src = { vertices: upload(mesh.vertices), faces: upload(mesh.faces) };
    const E = adj.count(src.faces, F, V);
    const out = { rowStart: dev.createBuffer({ size: Math.max(4 * (V + 1), 8) }), neighbours: dev.createBuffer({ size: Math.max(4 * E, 8) }), boundary: dev.createBuffer({ size: Math.max(4 * V, 8) }),
      smoothed: dev.createBuffer({ size: Math.max(12 * V, 8) }), normals: dev.createBuffer({ size: Math.max(12 * V, 8) }) };
    adj.emit(out.rowStart, out.neighbours, out.boundary, E);
    adj.normals(src.vertices, src.faces, V, F, out.normals);
    adj.smooth(src.vertices, out.smoothed, V, c.iterations, opt);
    const stats = adj.stats();
    const entry = { device: digest({ rowStart: new Uint32Array(bytes(out.rowStart, 4 * (V + 1))), neighbours: new Uint32Array(bytes(out.neighbours, 4 * E)),
      boundary: new Uint32Array(bytes(out.boundary, 4 * V)), smoothed: new Float32Array(bytes(out.smoothed, 12 * V)), normals: new Float32Array(bytes(out.normals, 12 * V)), stats }) };
    const one = hip.meshAdjacency(dev, mesh), smoothed = hip.smoothMesh(dev, mesh, c.iterations, opt);
    entry.host = digest({ rowStart: one.rowStart, neighbours: one.neighbours, boundary: one.boundary, smoothed: smoothed.vertices, normals: hip.vertexNormals(dev, mesh),
      stats: smoothed.stats });
    if (smoothed.faces !== mesh.faces || JSON.stringify(one.stats) !== JSON.stringify(stats)) errors.push(`${c.name}: the one-call forms`);
    entry.stats = stats;
    hip.destroyBuffers(out);
    hip.destroyBuffers(src);
    meshes[c.name] = entry;
  }

  // 2. refusals, and smoothing in place
  const vertices = upload(Float32Array.from([0, 0, 0, 1, 0, 0.25, 0, 1, 0.5, 1, 1, -0.5])), faces = upload(Uint32Array.from([0, 1, 2, 2, 1, 3]));
  const fresh = new hip.MeshAdjacency(dev), target = dev.createBuffer({ size: 48 }), room = dev.createBuffer({ size: 40 });
  refused('stats before count', 'WDGS_E_STATE', () => fresh.stats());
  refused('smooth before count', 'WDGS_E_STATE', () => fresh.smooth(vertices, target, 4, 1));
  if (fresh.count(faces, 2, 4) !== 10 || fresh.stats().boundaryEdges !== 4) errors.push(`two triangles: ${JSON.stringify(fresh.stats())}`);
  refused('too little room', 'WDGS_E_CAPACITY', () => fresh.emit(null, room, null, 9));
  refused('another vertex count', 'WDGS_E_STATE', () => fresh.smooth(vertices, target, 3, 1));
  refused('a NaN weight', 'WDGS_E', () => fresh.smooth(vertices, target, 4, 1, { lambda: NaN }));
  refused('too many iterations', 'WDGS_E', () => fresh.smooth(vertices, target, 4, 1025));
  fresh.smooth(vertices, target, 4, 3, { pinBoundary: false });
  fresh.smooth(vertices, vertices, 4, 3, { pinBoundary: false });
  if (sha([new Float32Array(dev.readBuffer(target, 48))]) !== sha([new Float32Array(dev.readBuffer(vertices, 48))])) errors.push('smoothing in place differs');
  fresh.destroy();
  [vertices, faces, target, room].forEach((b) => b.destroy());
  adj.destroy();

  // 3. two spheres in a volume
  const vol = new hip.TSDFVolume(dev, meta.volume.origin, meta.volume.voxel_size, meta.volume.dims, { truncation: meta.volume.truncation, colour: true });
  dev.queue.writeBuffer(vol.getTSDFBuffer(), 0, readAs('volume.tsdf.f32', Float32Array));
  dev.queue.writeBuffer(vol.getWeightBuffer(), 0, readAs('volume.weight.f32', Float32Array));
  dev.queue.writeBuffer(vol.getColourBuffer(), 0, readAs('volume.rgb.f32', Float32Array));
  const cell = meta.volume.cell, n = meta.volume.smooth;
  const plain = vol.extractMesh();
  const withNormals = vol.extractMesh(null, { weld: 'device', smooth: n, normals: true });
  const spheres = { plain: meshDigest(plain), defaults: meshDigest(vol.extractMesh(null, { weld: 'device', smooth: null, normals: false })),
    host: meshDigest(vol.extractMesh(null, { smooth: n, normals: true })), device: meshDigest(withNormals),
    ofMesh: meshDigest(Object.assign(hip.smoothMesh(dev, plain, n), { normals: hip.vertexNormals(dev, hip.smoothMesh(dev, plain, n)) })),
    simplifiedHost: meshDigest(vol.extractMesh(null, { smooth: n, simplify: cell, normals: true })),
    simplifiedDevice: meshDigest(vol.extractMesh(null, { weld: 'device', smooth: n, simplify: cell, normals: true })),
    ply: crypto.createHash('sha256').update(loaders.meshPLYBytes(withNormals)).digest('hex'), plyPlain: crypto.createHash('sha256').update(loaders.meshPLYBytes(plain)).digest('hex') };
  if (Object.keys(plain).join() !== 'vertices,faces,colours,keys') errors.push(`the defaults add keys: ${Object.keys(plain).join()}`);
  vol.destroy();

  const out = { errors, meshes, spheres };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHSMOOTH_RUN_OK');
}

main();
