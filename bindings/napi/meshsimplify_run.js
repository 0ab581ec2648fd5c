// node bindings/napi/meshsimplify_run.js <dir> -- simplification by vertex clustering through the node host (tests/test_gpu_meshsimplify_napi.py): every
// mesh of meta.json (<name>.vertices.f32, <name>.faces.u32, <name>.colours.u8 when it has colours, raw little-endian, with its origin and cell size) goes
// through simplifyMesh, as typed arrays and as device buffers; the volume of <dir> (two spheres) is written through the TSDFVolume getters, extracted with
// options.simplify under both welds and its device-simplified buffers are labelled and sampled.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const STATS = ['clusters', 'invalid', 'outside', 'collapsed', 'duplicate', 'vertices', 'faces'];
// one digest over the arrays in a fixed order, then the counts as u32 (tests/meshsimplify_ref.py: digest)
const digest = (r) => {
  const h = crypto.createHash('sha256');
  for (const k of ['vertices', 'faces', 'colours', 'keys', 'faceMap', 'vertexCluster']) if (r[k]) h.update(Buffer.from(r[k].buffer, r[k].byteOffset, r[k].byteLength));
  const counts = Uint32Array.from(STATS, (k) => r.stats[k]);
  h.update(Buffer.from(counts.buffer));
  return h.digest('hex');
};

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (a) => { const b = dev.createBuffer({ size: Math.max(a.byteLength, 8) }); if (a.byteLength) dev.queue.writeBuffer(b, 0, a); return b; };
  const bytes = (b, n) => (n ? dev.readBuffer(b, n) : new ArrayBuffer(0));

  // 1. the crafted meshes: the one-call form on typed arrays (colours come back as rgb), then on device buffers with every array read back (rgba)
  const meshes = {};
  for (const c of meta.meshes) {
    const mesh = { vertices: readAs(`${c.name}.vertices.f32`, Float32Array), faces: readAs(`${c.name}.faces.u32`, Uint32Array),
      colours: c.colours ? readAs(`${c.name}.colours.u8`, Uint8Array) : null };
    const entry = { host: digest(hip.simplifyMesh(dev, mesh, c.cell, { origin: c.origin })) };
    const src = { vertices: upload(mesh.vertices), faces: upload(mesh.faces), colours: mesh.colours ? upload(mesh.colours) : null,
      numVertices: mesh.vertices.length / 3, numFaces: mesh.faces.length / 3 };
    const b = hip.simplifyMesh(dev, src, c.cell, { origin: c.origin, asBuffers: true });
    const nv = b.numVertices, nf = b.numFaces;
    entry.device = digest({ vertices: new Float32Array(bytes(b.vertices, 12 * nv)), faces: new Uint32Array(bytes(b.faces, 12 * nf)),
      colours: b.colours ? new Uint8Array(bytes(b.colours, 4 * nv)) : null, keys: new BigUint64Array(bytes(b.keys, 8 * nv)),
      faceMap: new Uint32Array(bytes(b.faceMap, 4 * nf)), vertexCluster: new Uint32Array(bytes(b.vertexCluster, 4 * src.numVertices)), stats: b.stats });
    entry.stats = b.stats;
    if (b.vertices.size !== 12 * nv || b.faces.size !== 12 * nf || b.keys.size !== 8 * nv) errors.push(`${c.name}: asBuffers sizes`);
    hip.destroyBuffers(b);
    hip.destroyBuffers(src);
    meshes[c.name] = entry;
  }

  // 2. two spheres in a volume
  const vol = new hip.TSDFVolume(dev, meta.volume.origin, meta.volume.voxel_size, meta.volume.dims, { truncation: meta.volume.truncation, colour: true });
  dev.queue.writeBuffer(vol.getTSDFBuffer(), 0, readAs('volume.tsdf.f32', Float32Array));
  dev.queue.writeBuffer(vol.getWeightBuffer(), 0, readAs('volume.weight.f32', Float32Array));
  dev.queue.writeBuffer(vol.getColourBuffer(), 0, readAs('volume.rgb.f32', Float32Array));
  const cell = meta.volume.cell;
  const plain = vol.extractMesh();
  const spheres = { host: digest(vol.extractMesh(null, { simplify: cell })), device: digest(vol.extractMesh(null, { weld: 'device', simplify: cell })),
    ofMesh: digest(hip.simplifyMesh(dev, plain, cell, { origin: meta.volume.origin })), plainFaces: plain.faces.length / 3 };
  const tri = vol.extractTriangleBuffers();
  const welded = hip.weldTrianglesDevice(dev, tri, { asBuffers: true });
  hip.destroyBuffers(tri);
  vol.destroy();
  const simplified = hip.simplifyMesh(dev, welded, cell, { origin: meta.volume.origin, asBuffers: true });
  hip.destroyBuffers(welded);
  const onDevice = { vertices: simplified.vertices, faces: simplified.faces };
  spheres.faces = simplified.numFaces;
  spheres.components = hip.meshComponents(dev, onDevice).count;
  const samples = hip.sampleMesh(dev, onDevice, 50.0, 3);
  spheres.samples = crypto.createHash('sha256').update(Buffer.from(samples.points.buffer, samples.points.byteOffset, samples.points.byteLength)).digest('hex');
  hip.destroyBuffers(simplified);

  // 3. refusals
  const simp = new hip.MeshSimplifier(dev);
  const vertices = upload(Float32Array.from([0.5, 0.5, 0.5, 1.5, 0.5, 0.5, 0.5, 1.5, 0.5])), faces = upload(Uint32Array.from([0, 1, 2, 1, 2, 0]));
  const vout = dev.createBuffer({ size: 36 }), fout = dev.createBuffer({ size: 24 });
  refused('stats before count', 'WDGS_E_STATE', () => simp.stats());
  refused('emit before count', 'WDGS_E_STATE', () => simp.emit(vertices, 3, faces, 2, null, vout, fout));
  refused('a cell size of zero', 'WDGS_E', () => simp.count(vertices, 3, faces, 2, null, [0, 0, 0], 0));
  refused('a NaN origin', 'WDGS_E', () => simp.count(vertices, 3, faces, 2, null, [0, NaN, 0], 1));
  refused('a device mesh without an origin', undefined, () => hip.simplifyMesh(dev, { vertices, faces }, 1));
  const n = simp.count(vertices, 3, faces, 2, null, [0, 0, 0], 1);
  if (n.vertices !== 3 || n.faces !== 1 || simp.stats().duplicate !== 1) errors.push(`two rotations of one face: ${JSON.stringify(simp.stats())}`);
  refused('too little room', 'WDGS_E_CAPACITY', () => simp.emit(vertices, 3, faces, 2, null, vout, fout, null, null, null, null, 2, 1));
  refused('a count of other faces', 'WDGS_E_STATE', () => simp.emit(vertices, 3, faces, 1, null, vout, fout));
  simp.emit(vertices, 3, faces, 2, null, vout, fout);
  const kept = Array.from(new Uint32Array(dev.readBuffer(fout, 12)));
  if (kept.join() !== '0,1,2') errors.push(`two rotations of one face: kept ${kept.join()}`);
  simp.destroy();
  [vertices, faces, vout, fout].forEach((b) => b.destroy());

  const out = { errors, meshes, spheres };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHSIMPLIFY_RUN_OK');
}

main();
