// node bindings/napi/eval_run.js <dir> -- drives bindings/ts/trainer.js's held-out evaluation over the N-API addon on a cloud and a dataset written
// by tests/test_gpu_eval_napi.py: splits the views with loaders.holdoutSplit (meta.every), evaluates the test views and the training views, scores
// one image pair with imageSSIM / imageSSE directly, and writes the results to out.json for a bit-for-bit comparison with the Python host's.
'use strict';
const fs = require('fs');
const path = require('path');
const hip = require(path.join(__dirname, '..', 'ts', 'webdgs_hip.js'));
const loaders = require(path.join(__dirname, '..', 'ts', 'loaders.js'));
const { Trainer } = require(path.join(__dirname, '..', 'ts', 'trainer.js'));

const dir = process.argv[2];
const meta = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const u8 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Uint8Array(b.buffer, b.byteOffset, b.byteLength); };

function main() {
  const dev = new hip.HipDevice(0);
  const upload = (bytes) => { const b = dev.createBuffer({ size: bytes.byteLength }); dev.queue.writeBuffer(b, 0, bytes); return b; };
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
  const [trc, tri, tec, tei] = loaders.holdoutSplit(cameras, images, meta.every);
  const t = new Trainer(dev, undefined, { pipelineDepth: meta.pipeline_depth || 1 });
  t.setDensifyPruneConfig({ schedule: { enabled: false } });
  t.setPointCloud(pc);
  t.setDataset(trc, tri);
  t.setEvaluationViews(tec, tei);
  if (meta.eval_max_tile_entries) t.evalMaxTileEntries = meta.eval_max_tile_entries;
  t.start();
  const evalRes = t.evaluate();
  const trainRes = t.evaluate(meta.train_views, 'train');
  // one pair scored directly: the first two images, when they have one size
  const [a, b] = [images[0], images[1]];
  const direct = { sse: hip.imageSSE(dev, a.texture, b.texture, a.width * a.height), ssim: hip.imageSSIM(dev, a.texture, b.texture, a.width, a.height) };
  const f64hex = (x) => Buffer.from(new Float64Array([x]).buffer).toString('hex');
  const pack = (r) => ({ views: r.views, sse: r.sse, ssim_hex: r.ssim.map(f64hex), psnr: r.psnr.map((x) => (Number.isFinite(x) ? x : String(x))),
    mean_ssim_hex: f64hex(r.mean_ssim), iteration: r.iteration });
  fs.writeFileSync(path.join(dir, 'out.json'), JSON.stringify({ split: [trc.length, tec.length], eval: pack(evalRes), train: pack(trainRes),
    direct: { sse: direct.sse, ssim_hex: f64hex(direct.ssim) } }));
  t.destroy();
  dev.destroy();
  console.log('EVAL_RUN_OK');
}

main();
