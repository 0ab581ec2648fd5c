// node bindings/napi/contrib_run.js <dir> -- per-Gaussian render contribution and contribution-based pruning through the node host
// (tests/test_gpu_contrib_napi.py).  meta.mode 'scene': the synthetic scene of meta.config (bindings/ts/synth.js generates the very bits
// webdgs_amd/synth.py does) under meta.cameras cameras of a circle -- TiledRasterizer.encodeContribution over the views into one buffer, then
// DensifyPrunePass.encodeContributionDecision (minPixels 1), prefix sum, total and scatter into a new cloud.  meta.mode 'trainer': a cloud and a dataset
// written by the test -- Trainer.contributionStats, then Trainer.pruneByContribution({ minPixels: 1 }).  The records and the pruned cloud go back as
// raw files, for a byte-for-byte comparison with the Python host's.
'use strict';
const fs = require('fs');
const path = require('path');
const ts = (m) => require(path.join(__dirname, '..', 'ts', m));
const hip = ts('webdgs_hip.js'), synth = ts('synth.js');
const { Trainer } = ts('trainer.js');

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const u8 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Uint8Array(b.buffer, b.byteOffset, b.byteLength); };
const put = (name, raw) => fs.writeFileSync(path.join(dir, name), Buffer.from(raw));

function scene(dev, upload) {
  const cfg = meta.config, n = cfg.num_points;
  const s = synth.makeGaussians(cfg), cams = synth.circleCameras(cfg, meta.cameras);
  const pc = { type: 'full', num_points: n, sh_deg: cfg.sh_deg, gaussian_3d_buffer: upload(s.gaussians), sh_buffer: upload(s.sh) };
  const cbuf = upload(cams[0]);
  const fwd = new hip.TiledForwardPass(dev, pc, cbuf, { viewportWidth: cfg.width, viewportHeight: cfg.height, renderMode: 'gaussian' });
  const rast = new hip.TiledRasterizer({ device: dev, forwardPass: fwd, format: 'rgba8unorm' });
  const dp = new hip.DensifyPrunePass(dev);
  const errors = [];
  // (the addon names WDGS_E_STATE and WDGS_E_CAPACITY; every other code is 'WDGS_E' with the number in the message: -1 is WDGS_E_INVALID)
  const refused = (what, code, f) => {
    try { f(); errors.push(`${what}: not refused`); } catch (e) {
      const got = e.code === 'WDGS_E' && String(e.message).startsWith('[wdgs -1]') ? 'WDGS_E_INVALID' : e.code;
      if (got !== code) errors.push(`${what}: ${e.code || ''} ${e.message || e}`);
    }
  };
  const stats = hip.createContributionBuffer(dev, n);
  refused('encodeContribution before encode', 'WDGS_E_STATE', () => rast.encodeContribution(null, stats));
  for (const cam of cams) {
    dev.queue.writeBuffer(cbuf, 0, cam);
    fwd.encode(null);
    rast.encode(null, cfg.width, cfg.height);
    rast.encodeContribution(null, stats);
  }
  put('out_stats.bin', dev.readBuffer(stats, 16 * n));
  refused('an all-zero rule', 'WDGS_E_INVALID', () => dp.encodeContributionDecision(null, n, stats, {}));
  dp.ensureSize(n);
  dp.encodeContributionDecision(null, n, stats, { minPixels: 1 });
  const offsets = dp.encodePrefixSum(null);
  dp.encodeTotalOut(null);
  const total = dp.readTotal();
  const out = hip.allocatePointCloudLike(dev, pc, { numPoints: total });
  dp.encodeScatter(null, { pointCloud: pc, outOffsetBuffer: offsets, outNumPoints: total, resetNewOptimizerState: false }, { outPointCloud: out });
  dev.synchronize();
  put('out_gaussians.bin', dev.readBuffer(out.gaussian_3d_buffer, 24 * total));
  put('out_sh.bin', dev.readBuffer(out.sh_buffer, 96 * total));
  for (const b of [out.gaussian_3d_buffer, out.sh_buffer, stats]) b.destroy();
  dp.destroy(); rast.destroy(); fwd.destroy(); cbuf.destroy();
  pc.gaussian_3d_buffer.destroy(); pc.sh_buffer.destroy();
  return { errors, total };
}

function trainer(dev, upload) {
  const pc = { type: 'full', num_points: meta.num_points, sh_deg: meta.sh_deg, gaussian_3d_buffer: upload(u8('gaussians.bin')), sh_buffer: upload(u8('sh.bin')) };
  const camBytes = u8('cameras.bin'), imgBytes = u8('images.bin');
  const cams = new Float32Array(camBytes.buffer.slice(camBytes.byteOffset, camBytes.byteOffset + camBytes.byteLength));
  const cameras = [], images = [];
  let at = 0;
  meta.sizes.forEach(([w, h], v) => {
    cameras.push({ camera: cams.slice(v * 68, v * 68 + 68), width: w, height: h });
    images.push({ texture: upload(imgBytes.subarray(at, at + 4 * w * h)), width: w, height: h });
    at += 4 * w * h;
  });
  const t = new Trainer(dev, undefined, {});
  t.setDensifyPruneConfig({ schedule: { enabled: false } });
  t.setPointCloud(pc);
  t.setDataset(cameras, images);
  t.start();
  const errors = [];
  try { t.pruneByContribution({}); errors.push('no criterion: not refused'); } catch (e) { /* expected */ }
  const s = t.contributionStats();
  put('out_sum_q.bin', s.sum_q.buffer); put('out_max_weight.bin', s.max_weight.buffer); put('out_pixels.bin', s.pixels.buffer);
  const some = t.contributionStats(meta.some_views);
  put('out_some_pixels.bin', some.pixels.buffer);
  const r = t.pruneByContribution({ minPixels: 1 });
  const n = t.getPointCount();
  put('out_gaussians.bin', dev.readBuffer(t.pointCloud.gaussian_3d_buffer, 24 * n));
  put('out_sh.bin', dev.readBuffer(t.pointCloud.sh_buffer, 96 * n));
  const sse = t.evaluate(null, 'train').sse;
  t.destroy();
  return { errors, result: r, views: s.views, some_views: some.views, points: n, sse };
}

function main() {
  const dev = new hip.HipDevice(0);
  const upload = (words) => { const b = dev.createBuffer({ size: words.byteLength }); dev.queue.writeBuffer(b, 0, words); return b; };
  const out = meta.mode === 'trainer' ? trainer(dev, upload) : scene(dev, upload);
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify(out));
  dev.destroy();
  console.log('CONTRIB_RUN_OK');
}

main();
