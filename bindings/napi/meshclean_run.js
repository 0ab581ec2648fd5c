// node bindings/napi/meshclean_run.js <dir> -- mesh connected components and small-component removal through the node host
// (tests/test_gpu_meshclean_napi.py): every mesh of meta.json (<name>.vertices.f32, <name>.faces.u32, raw little-endian) goes through meshComponents and,
// for each of its selections, removeSmallComponents; the volume of <dir> (two spheres) is written through the TSDFVolume getters, extracted, labelled
// and reduced to its largest component.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const digest = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const labelDigests = (r) => ({ count: r.count, invalidFaces: r.invalidFaces, faceComponent: digest(r.faceComponent), vertexComponent: digest(r.vertexComponent),
  triangles: digest(r.triangles), vertices: digest(r.vertices) });
const meshDigests = (m) => {
  const out = { vertices: digest(m.vertices), faces: digest(m.faces), vertexMap: digest(m.vertexMap), faceMap: digest(m.faceMap), components: digest(m.components) };
  if (m.colours) out.colours = digest(m.colours);
  if (m.keys) out.keys = digest(m.keys);
  return out;
};

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };

  // 1. the meshes
  const meshes = {};
  for (const m of meta.meshes) {
    const mesh = { vertices: readAs(`${m.name}.vertices.f32`, Float32Array), faces: readAs(`${m.name}.faces.u32`, Uint32Array) };
    const labels = hip.meshComponents(dev, mesh);
    const entry = { labels: labelDigests(labels), kept: {} };
    m.selections.forEach((sel, i) => {
      if (!hip.selectComponents(labels.triangles, sel).some((k) => k) && sel.keepLargest !== 0) errors.push(`${m.name}: selection ${i} keeps nothing`);
      entry.kept[String(i)] = meshDigests(hip.removeSmallComponents(dev, mesh, sel));
    });
    meshes[m.name] = entry;
  }

  // 2. two spheres in a volume
  const vol = new hip.TSDFVolume(dev, meta.volume.origin, meta.volume.voxel_size, meta.volume.dims, { truncation: meta.volume.truncation, colour: true });
  dev.queue.writeBuffer(vol.getTSDFBuffer(), 0, readAs('volume.tsdf.f32', Float32Array));
  dev.queue.writeBuffer(vol.getWeightBuffer(), 0, readAs('volume.weight.f32', Float32Array));
  dev.queue.writeBuffer(vol.getColourBuffer(), 0, readAs('volume.rgb.f32', Float32Array));
  const two = vol.extractMesh();
  vol.destroy();
  const spheres = { labels: labelDigests(hip.meshComponents(dev, two)), kept: meshDigests(hip.removeSmallComponents(dev, two, { keepLargest: 1 })) };

  // 3. refusals
  const comp = new hip.MeshComponents(dev);
  refused('read before label', 'WDGS_E_STATE', () => comp.read());
  refused('select before label', 'WDGS_E_STATE', () => comp.select([1]));
  refused('2^31 vertices', 'WDGS_E', () => comp.label(null, 0, 2 ** 31));
  const faces = dev.createBuffer({ size: 12 });
  dev.queue.writeBuffer(faces, 0, Uint32Array.from([0, 1, 2]));
  if (comp.label(faces, 1, 3) !== 1) errors.push('one face: not one component');
  refused('compact before select', 'WDGS_E_STATE', () => comp.compact(null, null, faces));
  refused('a selection of the wrong length', 'WDGS_E', () => comp.select([1, 1]));
  comp.select([1]);
  refused('too little room', 'WDGS_E_CAPACITY', () => comp.compact(null, null, faces, null, null, 3, 0));
  comp.destroy();
  faces.destroy();

  const out = { errors, meshes, spheres };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHCLEAN_RUN_OK');
}

main();
