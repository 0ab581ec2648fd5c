// node bindings/napi/meshweld_run.js <dir> -- welding on the device through the node host (tests/test_gpu_meshweld_napi.py): every soup of meta.json
// (<name>.keys.u64, <name>.positions.f32, <name>.colours.u8, raw little-endian) goes through weldTrianglesDevice; the volume of <dir> (two spheres) is
// written through the TSDFVolume getters and extracted with the host weld and the device weld, and its device-welded buffers are reduced to their
// largest component.  SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const digest = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const meshDigests = (m) => {
  const out = {};
  for (const k of ['vertices', 'faces', 'vertexMap', 'faceMap', 'components', 'colours', 'keys']) if (m[k]) out[k] = digest(m[k]);
  return out;
};

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };

  // 1. the soups: the one-call form, and the welder's statistics
  const soups = {};
  for (const name of meta.soups) {
    const tri = { keys: readAs(`${name}.keys.u64`, BigUint64Array), positions: readAs(`${name}.positions.f32`, Float32Array), colours: readAs(`${name}.colours.u8`, Uint8Array) };
    const entry = meshDigests(hip.weldTrianglesDevice(dev, tri));
    const keys = dev.createBuffer({ size: Math.max(tri.keys.byteLength, 8) });
    if (tri.keys.byteLength) dev.queue.writeBuffer(keys, 0, tri.keys);
    const welder = new hip.MeshWelder(dev);
    entry.numVertices = welder.count(keys, tri.keys.length);
    entry.passesRun = welder.stats().passesRun;
    welder.destroy();
    keys.destroy();
    soups[name] = entry;
  }

  // 2. two spheres in a volume
  const vol = new hip.TSDFVolume(dev, meta.volume.origin, meta.volume.voxel_size, meta.volume.dims, { truncation: meta.volume.truncation, colour: true });
  dev.queue.writeBuffer(vol.getTSDFBuffer(), 0, readAs('volume.tsdf.f32', Float32Array));
  dev.queue.writeBuffer(vol.getWeightBuffer(), 0, readAs('volume.weight.f32', Float32Array));
  dev.queue.writeBuffer(vol.getColourBuffer(), 0, readAs('volume.rgb.f32', Float32Array));
  const host = vol.extractMesh(), device = vol.extractMesh(null, { weld: 'device' });
  const tri = vol.extractTriangleBuffers();
  const welded = hip.weldTrianglesDevice(dev, tri, { asBuffers: true });
  hip.destroyBuffers(tri);
  vol.destroy();
  const spheres = { host: meshDigests(host), device: meshDigests(device),
    kept: meshDigests(hip.removeSmallComponents(dev, { vertices: welded.vertices, faces: welded.faces }, { keepLargest: 1 })) };
  hip.destroyBuffers(welded);

  // 3. refusals
  const welder = new hip.MeshWelder(dev);
  const keys = dev.createBuffer({ size: 48 }), faces = dev.createBuffer({ size: 24 }), vertices = dev.createBuffer({ size: 72 });
  dev.queue.writeBuffer(keys, 0, BigUint64Array.from([5n, 3n, 9n, 3n, 0xFFFFFFFFFFFFFFFFn, 0n]));
  refused('stats before count', 'WDGS_E_STATE', () => welder.stats());
  refused('emit before count', 'WDGS_E_STATE', () => welder.emit(keys, 6, null, null, faces));
  refused('slots not three per triangle', 'WDGS_E', () => welder.count(keys, 5));
  refused('2^32 slots', 'WDGS_E', () => welder.count(keys, 2 ** 32));
  if (welder.count(keys, 6) !== 5) errors.push('six slots: not five vertices');
  refused('too little room', 'WDGS_E_CAPACITY', () => welder.emit(keys, 6, vertices, null, faces, vertices, null, null, 4));
  refused('a count of other slots', 'WDGS_E_STATE', () => welder.emit(keys, 3, null, null, faces));
  welder.emit(keys, 6, null, null, faces);
  const ranks = Array.from(new Uint32Array(dev.readBuffer(faces, 24)));
  if (ranks.join() !== '2,1,3,1,4,0') errors.push(`six slots: ranks ${ranks.join()}`);
  welder.destroy();
  [keys, faces, vertices].forEach((b) => b.destroy());

  const out = { errors, soups, spheres };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('MESHWELD_RUN_OK');
}

main();
