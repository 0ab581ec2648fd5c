// node bindings/napi/knn_run.js <dir> -- the k-nearest query and the neighbour-based scale initialisation through the node host
// (tests/test_gpu_knn_napi.py): the point set and queries of <dir> (raw little-endian files) go through PointIndex.kNearest for every k and cutoff of
// meta.json, the cloud of <dir> through initScalesFromNeighbours; SHA-256 digests of the outputs go to out.json and are printed.
'use strict';
const fs = require('fs');
const path = require('path');
const crypto = require('crypto');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const readAs = (name, Type) => { const b = fs.readFileSync(path.join(dir, name)); return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const digest = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');

function main() {
  const dev = new hip.HipDevice(0);
  const errors = [];
  const refused = (what, code, f) => { try { f(); errors.push(`${what}: not refused`); } catch (e) { if (e.code !== code) errors.push(`${what}: ${e.code || e}`); } };
  const upload = (words) => { const b = dev.createBuffer({ size: Math.max(words.byteLength, 4) }); if (words.byteLength) dev.queue.writeBuffer(b, 0, words); return b; };

  // 1. the k nearest, every k and cutoff
  const points = readAs('points.f32', Float32Array), queries = readAs('queries.f32', Float32Array);
  const index = new hip.PointIndex(dev, points, { cellSize: meta.cell_size });
  const knn = {};
  meta.cutoffs.forEach((cutoff, c) => {          // keyed "<position of the cutoff>/<k>"
    for (const k of meta.ks) {
      const r = index.kNearest(queries, k, cutoff);
      knn[`${c}/${k}`] = { d2: digest(r.d2), index: digest(r.index) };
    }
  });
  const self = index.kNearest(points, 3, meta.cutoffs[0], true);
  knn.self = { d2: digest(self.d2), index: digest(self.index) };
  refused('k = 0', 'WDGS_E', () => index.kNearest(queries, 0, 1));
  refused('k = 17', 'WDGS_E', () => index.kNearest(queries, 17, 1));
  refused('a cutoff of 0', 'WDGS_E', () => index.kNearest(queries, 3, 0));
  const bounds = index.bounds();
  index.destroy();

  // 2. the scales
  const scales = {};
  for (const [name, maxDistance] of [['default', null], ['small', meta.small_cutoff]]) {
    const pc = { type: 'normal', num_points: meta.num_points, sh_deg: 0, gaussian_3d_buffer: upload(readAs('gaussians.u32', Uint32Array)),
      sh_buffer: upload(readAs('sh.u32', Uint32Array)) };
    const r = hip.initScalesFromNeighbours(dev, pc, { k: 3, maxDistance });
    scales[name] = { gaussians: digest(new Uint32Array(dev.readBuffer(pc.gaussian_3d_buffer, 24 * meta.num_points))),
      sh: digest(new Uint32Array(dev.readBuffer(pc.sh_buffer, 96 * meta.num_points))), meanD2: digest(r.meanD2), found: digest(r.found) };
    pc.gaussian_3d_buffer.destroy(); pc.sh_buffer.destroy();
  }
  const out = { errors, knn, scales, bounds: { lo: Array.from(bounds.lo), hi: Array.from(bounds.hi) } };
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  console.log(JSON.stringify(out));
  dev.destroy();
  console.log('KNN_RUN_OK');
}

main();
