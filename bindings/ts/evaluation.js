'use strict';
/*
 * evaluation.js (+ evaluation.d.ts) -- `Evaluator`: everything a Trainer can measure about its model without training it -- held-out evaluation,
 * normal consistency, TSDF fusion and mesh extraction, geometry metrics, render contribution (webdgs_amd/evaluation.py is the Python host's; none of
 * it has a counterpart in the reference).  It renders through pass sets of its own (no backward pass), one per image size, built on first use and
 * following the trainer's cloud, and answers the capacity reports about them itself (CapacityReports.settle).  Trainer keeps the public methods and
 * delegates to its Evaluator.
 */
const hip = require('./webdgs_hip.js');
const { destroyPassSets } = require('./trainer.js');

/** hip.FaceVisibility's cumulative totals as per-view lists: the counted, agreeing and foreign pixels of each view. */
function perView(totals) {
  const per = (key) => totals.map((t, i) => t[key] - (i ? totals[i - 1][key] : 0));
  return { counted: per('countedPixels'), agreeing: per('agreeingPixels'), foreign: per('foreignPixels') };
}

/** The evaluation side of one Trainer.  It owns the evaluation views with their camera blocks (and the textures it uploaded itself), the per-size
 *  evaluation PassSets, the size an overflow has grown their tile-entry lists to and the long-list settings they were built with.
 *
 *  The seam -- the only members of the trainer used here:
 *    - device, pointCloud, iteration;
 *    - trainCameras, images, cameraBuffers: the training views, for split 'train';
 *    - newPassSet: carries the live SH-DC words and the trainer's long-list settings;  dcWords, longLists;
 *    - drain() and growTileEntryCapacity(): a training step still in flight is awaited, its overflow answered as step() would.
 *  Never the training or metric pass sets, the command buffers, the tickets, the random draws, the optimizer or the densify pass. */
class Evaluator {
  constructor(trainer) {
    this.trainer = trainer; this.device = trainer.device;
    this.cameras = []; this.images = []; this.cameraBuffers = []; this.ownedTextures = [];
    this.sets = new Map();
    this.maxTileEntries = 0;   // tile-entry lists of the evaluation passes (0: what the training passes get)
    this.tileEntries = 0;      // (what an overflowing evaluation view has made of them)
    this.longLists = null;
  }
  destroy() {
    this.destroySets();
    for (const b of this.cameraBuffers.concat(this.ownedTextures)) b.destroy();
    this.cameraBuffers = []; this.ownedTextures = [];
  }

  // ---------------------------------------------------------------- views and pass sets
  /** Views to evaluate on and never to train on (loaders.holdoutSplit gives the every-8th test views of the 3DGS convention).  Same shapes as
   *  setDataset; the images may have another size than the training images. */
  setEvaluationViews(cameras, images) {
    if (cameras.length !== images.length) throw new Error(`setEvaluationViews: ${cameras.length} cameras, ${images.length} images`);
    for (const b of this.cameraBuffers.concat(this.ownedTextures)) b.destroy();
    this.ownedTextures = [];
    const imgs = images.map((im) => {
      if (im.texture) return im;
      const tex = this.device.createBuffer({ size: 4 * im.width * im.height, label: 'eval image' });
      this.device.queue.writeBuffer(tex, 0, im.bitmap);
      this.ownedTextures.push(tex);
      return Object.assign({}, im, { texture: tex });
    });
    this.cameras = cameras.map((c, i) => (c.camera ? c : Object.assign({}, c, { camera: require('./loaders.js').cameraUniforms(c, imgs[i].width, imgs[i].height) })));
    this.images = imgs;
    this.cameraBuffers = this.cameras.map((c) => {
      const b = this.device.createBuffer({ size: 272, label: 'eval camera uniform' });
      this.device.queue.writeBuffer(b, 0, c.camera);
      return b;
    });
  }
  destroySets() { destroyPassSets(this.sets.values()); this.sets = new Map(); }
  /** The pass set (no backward pass) for one image size, built through the trainer's newPassSet (live SH-DC words, its long-list settings).  Never a guard. */
  set(w, h, cam) {
    const key = `${w}x${h}`;
    if (!this.sets.has(key)) this.sets.set(key, this.trainer.newPassSet(cam, w, h, false, this.tileEntries || this.maxTileEntries || null));
    return this.sets.get(key);
  }
  followCloud() {
    const t = this.trainer;
    if (JSON.stringify(this.longLists) !== JSON.stringify(t.longLists)) {
      this.destroySets();
      this.longLists = t.longLists ? Object.assign({}, t.longLists) : null;
    }
    for (const { forwardPass: fw } of this.sets.values()) {
      if (fw.pointCloud !== t.pointCloud && !fw.setPointCloud(t.pointCloud)) { this.destroySets(); break; }
    }
    for (const s of this.sets.values()) s.forwardPass.setDcSource(t.dcWords);
  }
  /** Waits for the evaluation renders; the entries the largest overflowing one needed, or null (other owners' lines are left for them). */
  overflow() {
    const { mine } = this.device.capacityReports.settle([...this.sets.values()].map((s) => s.forwardPass.handle), () => this.device.synchronize());
    return mine.length ? Math.max(...mine.map((o) => o.needed)) : null;
  }
  /** { cams, imgs, bufs, ids } of a split, checked: what evaluate, normalConsistency and contributionStats start with. */
  views(what, viewIds, split) {
    const t = this.trainer;
    if (split !== 'eval' && split !== 'train') throw new Error(`${what}: split must be 'eval' or 'train', not ${split}`);
    if (!t.pointCloud) throw new Error(`${what}: no point cloud`);
    const [cams, imgs, bufs] = split === 'eval' ? [this.cameras, this.images, this.cameraBuffers] : [t.trainCameras, t.images, t.cameraBuffers];
    const ids = viewIds === undefined || viewIds === null ? cams.map((_, i) => i) : viewIds.map((v) => Math.floor(v));
    for (const v of ids) if (!(v >= 0 && v < cams.length)) throw new RangeError(`${what}: view ${v} of ${cams.length} (${split})`);
    return { cams, imgs, bufs, ids };
  }
  /** Drains the trainer's pipeline in front of renders through the evaluation passes (a training step's overflow is met as step() would have met it). */
  drain() { try { this.trainer.drain(); } catch (e) { if (!this.trainer.growTileEntryCapacity(e)) throw e; } }

  /** The render loop: every view of `ids` through the evaluation pass set of its size, then each(i, v, passSet, width, height); after an overflow the
   *  lists are grown, restart() is called and ALL views are rendered again. */
  renderViews(ids, imgs, bufs, each, restart, what) {
    while (ids.length) {
      this.followCloud();
      ids.forEach((v, i) => {
        const im = imgs[v], w = im.width, h = im.height;
        const s = this.set(w, h, bufs[v]);
        s.forwardPass.setCameraBuffer(bufs[v]);
        s.forwardPass.encode(null);
        s.rasterizer.encode(null, w, h);
        each(i, v, s, w, h);
      });
      const needed = this.overflow();
      if (needed === null) break;
      const now = Math.max(this.tileEntries, ...[...this.sets.values()].map((s) => Number(s.forwardPass.getResources().maxTileEntries)));
      const next = hip.grownTileEntries(now, needed);
      if (next <= now) throw new Error(`${what}: a view needs ${needed} tile entries, more than the lists can hold`);
      console.warn(`evaluation tile-entry lists grown from ${now} to ${next} entries after an overflow; the views are rendered again`);
      this.tileEntries = next;
      this.destroySets();
      if (restart) restart();
    }
  }

  // ---------------------------------------------------------------- held-out evaluation
  /** PSNR and SSIM of the current model on the evaluation views (split 'eval') or on training views (split 'train'): { iteration, views, psnr, ssim,
   *  sse, mean_psnr, mean_ssim, ms }.  Drains the pipeline, renders every view through passes of its own, writes view i's SSE and SSIM into slot i
   *  of two device arrays and reads them back once; a view that overflowed its tile-entry lists is rendered again with larger lists.  Training is
   *  untouched (no random draw, no training pass, no recording dropped).  Per rank, no collective.  Same results as the Python host's. */
  evaluate(viewIds, split) {
    const { imgs, bufs, ids } = this.views('evaluate', viewIds, split || 'eval');
    const t0 = Date.now();
    this.drain();
    const n = ids.length, slots = Math.max(1, n);
    const out = this.device.createBuffer({ size: 16 * slots, label: 'evaluation sse + ssim' });
    let raw;
    try {
      this.renderViews(ids, imgs, bufs, (i, v, s, w, h) => {
        const pred = s.rasterizer.getOutputTextureView();
        hip.encodeImageSSE(this.device, pred, imgs[v].texture, w * h, this.device.view(out.ptr + BigInt(8 * i), 8));
        hip.encodeImageSSIM(this.device, pred, imgs[v].texture, w, h, this.device.view(out.ptr + BigInt(8 * (slots + i)), 8));
      }, null, 'evaluate');
      raw = n ? this.device.readBuffer(out, 16 * slots) : new ArrayBuffer(16);
    } finally { out.destroy(); }
    const sse = [...new BigUint64Array(raw, 0, n)].map(Number);
    const ssim = [...new Float64Array(raw, 8 * slots, n)];
    const psnr = ids.map((v, i) => hip.psnrFromSSE(sse[i], imgs[v].width * imgs[v].height));
    const mean = (a) => (a.length ? a.reduce((x, y) => x + y, 0) / a.length : NaN);
    return { iteration: this.trainer.iteration, views: ids, psnr, ssim, sse, mean_psnr: mean(psnr), mean_ssim: mean(ssim), ms: Date.now() - t0 };
  }

  // ---------------------------------------------------------------- normal consistency (DESIGN.md section 12)
  /** How well the composited normals of the current model agree with the normals of its own depth map, per view: { iteration, views, value, pixels,
   *  sum_e, sum_a, mean, ms } -- value[i] the weight-averaged 1 - cos of normalAgreement between encodeNormal's image and depthToNormals of the
   *  `depthKind` ('median' | 'expected') depth image, mean the same average over all views' pixels.  Rendered through evaluate's passes with its
   *  isolation; evaluate()'s result is what it was.  Same results as the Python host's. */
  normalConsistency(viewIds, split, depthKind) {
    split = split || 'eval'; depthKind = depthKind || 'median';
    if (depthKind !== 'median' && depthKind !== 'expected') throw new Error(`normalConsistency: depthKind must be 'median' or 'expected', not ${depthKind}`);
    const { cams, imgs, bufs, ids } = this.views('normalConsistency', viewIds, split);
    const t0 = Date.now();
    this.drain();
    const n = ids.length, slots = Math.max(1, n);
    const out = this.device.createBuffer({ size: 24 * slots, label: 'normal agreement sums' });
    const scratch = this.device.createBuffer({ size: 16 * Math.max(1, ...ids.map((v) => imgs[v].width * imgs[v].height)), label: 'depth normals' });
    let raw;
    try {
      this.renderViews(ids, imgs, bufs, (i, v, s, w, h) => {
        s.rasterizer.encodeDepth(null, [depthKind]);
        s.rasterizer.encodeNormal(null);
        hip.depthToNormals(this.device, s.rasterizer.getDepthTextureView(depthKind), w, h, cams[v].camera, scratch);
        hip.encodeNormalAgreement(this.device, s.rasterizer.getNormalTextureView(), scratch, w, h, this.device.view(out.ptr + BigInt(24 * i), 24));
      }, null, 'normalConsistency');
      raw = n ? this.device.readBuffer(out, 24 * slots) : new ArrayBuffer(24);
    } finally { scratch.destroy(); out.destroy(); }
    const sums = [...new BigUint64Array(raw, 0, 3 * n)].map(Number);
    const col = (k) => ids.map((_, i) => sums[3 * i + k]);
    const sum_e = col(0), sum_a = col(1), pixels = col(2), total = (a) => a.reduce((x, y) => x + y, 0);
    return { iteration: this.trainer.iteration, views: ids, value: sum_e.map((e, i) => (sum_a[i] ? e / sum_a[i] : NaN)), pixels, sum_e, sum_a,
      mean: total(sum_a) ? total(sum_e) / total(sum_a) : NaN, ms: Date.now() - t0 };
  }

  // ---------------------------------------------------------------- a mesh against the model's own depth maps (DESIGN.md section 20)
  /** How far `mesh` (hip.rasterizeMesh's: typed arrays or an object of HipBuffers) agrees with the model it came from, view by view, with no reference
   *  geometry: per view the model's depthKind depth map (b; present where its weight sum is at least minWeightSum) against the mesh rasterized under the same
   *  camera (a), through hip.encodeDepthAgreement.  options: { viewIds, split = 'eval', depthKind = 'median', maxDifference = 1, threshold = 0.05,
   *  minWeightSum = 0.5, near, cull }.  Returns { iteration, views, both, onlyA, onlyB, within, sum_q, mean (one entry per view), total, ms }: onlyB pixels are
   *  where the model sees surface and the mesh has a hole.  Rendered through evaluate's passes with its isolation.  Same results as the Python host's. */
  meshDepthAgreement(mesh, options) {
    const o = options || {}, split = o.split || 'eval', depthKind = o.depthKind || 'median';
    const maxDifference = o.maxDifference === undefined ? 1.0 : o.maxDifference, threshold = o.threshold === undefined ? 0.05 : o.threshold;
    const minWeightSum = o.minWeightSum === undefined ? 0.5 : o.minWeightSum;
    if (depthKind !== 'median' && depthKind !== 'expected') throw new Error(`meshDepthAgreement: depthKind must be 'median' or 'expected', not ${depthKind}`);
    const { imgs, bufs, ids } = this.views('meshDepthAgreement', o.viewIds, split);
    const t0 = Date.now();
    this.drain();
    const dev = this.device, n = ids.length, slots = Math.max(1, n);
    const src = hip.meshOnDevice(dev, mesh, 'meshDepthAgreement');
    const out = dev.createBuffer({ size: 40 * slots, label: 'depth agreement sums' });
    const scratch = dev.createBuffer({ size: 4 * Math.max(1, ...ids.map((v) => imgs[v].width * imgs[v].height)), label: 'mesh depth' });
    const rasterizer = new hip.MeshRasterizer(dev);
    let raw;
    try {
      if (n) {   // (grown once, to the largest view, in front of the loop)
        const big = ids.reduce((a, v) => (imgs[v].width * imgs[v].height > imgs[a].width * imgs[a].height ? v : a), ids[0]);
        rasterizer.encode(src.vertices, src.V, src.faces, src.F, null, bufs[ids[0]], imgs[big].width, imgs[big].height, { near: o.near, cull: o.cull, depth: scratch });
      }
      this.renderViews(ids, imgs, bufs, (i, v, s, w, h) => {
        s.rasterizer.encodeDepth(null, [depthKind, 'weight_sum']);
        rasterizer.encode(src.vertices, src.V, src.faces, src.F, null, bufs[v], w, h, { near: o.near, cull: o.cull, depth: scratch });
        hip.encodeDepthAgreement(dev, scratch, s.rasterizer.getDepthTextureView(depthKind), w, h, maxDifference, threshold, dev.view(out.ptr + BigInt(40 * i), 40),
          { bWeightSum: s.rasterizer.getDepthTextureView('weight_sum'), minWeightSum });
      }, null, 'meshDepthAgreement');
      raw = n ? dev.readBuffer(out, 40 * slots) : new ArrayBuffer(40);
    } finally {
      rasterizer.destroy(); scratch.destroy(); out.destroy();
      if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
    }
    const sums = [...new BigUint64Array(raw, 0, 5 * n)].map(Number);
    const per = ids.map((_, i) => hip.depthAgreementResult(sums.slice(5 * i, 5 * i + 5), maxDifference));
    const result = { iteration: this.trainer.iteration, views: ids };
    for (const k of ['both', 'onlyA', 'onlyB', 'within', 'sum_q', 'mean']) result[k] = per.map((p) => p[k]);
    result.total = hip.depthAgreementResult([0, 1, 2, 3, 4].map((k) => ids.reduce((a, _, i) => a + sums[5 * i + k], 0)), maxDifference);
    result.ms = Date.now() - t0;
    return result;
  }

  // ---------------------------------------------------------------- which faces of a mesh the views see (DESIGN.md section 21)
  /** { visibility, ids, totals }: a hip.FaceVisibility of the mesh on the device (src: hip.meshOnDevice's) accumulated over the views -- the caller destroys
   *  it -- and its cumulative totals after each view.  meshDepthAgreement's loop: the rasterizer grown once, one encode and one accumulate per view. */
  faceVisibilityOver(what, src, o) {
    const split = o.split || 'train', depthKind = o.depthKind || 'median';
    const threshold = o.threshold === undefined || o.threshold === null ? 0.05 : o.threshold, minWeightSum = o.minWeightSum === undefined || o.minWeightSum === null ? 0.5 : o.minWeightSum;
    if (depthKind !== 'median' && depthKind !== 'expected') throw new Error(`${what}: depthKind must be 'median' or 'expected', not ${depthKind}`);
    const { imgs, bufs, ids } = this.views(what, o.viewIds, split);
    this.drain();
    const dev = this.device, npix = Math.max(4, ...ids.map((v) => imgs[v].width * imgs[v].height));
    const depth = dev.createBuffer({ size: 4 * npix, label: 'mesh depth' }), image = dev.createBuffer({ size: 4 * npix, label: 'mesh face image' });
    const rasterizer = new hip.MeshRasterizer(dev), visibility = new hip.FaceVisibility(dev), totals = [];
    try {
      visibility.reset(src.F);
      if (ids.length) {   // (grown once, to the largest view, in front of the loop)
        const big = ids.reduce((a, v) => (imgs[v].width * imgs[v].height > imgs[a].width * imgs[a].height ? v : a), ids[0]);
        rasterizer.encode(src.vertices, src.V, src.faces, src.F, null, bufs[ids[0]], imgs[big].width, imgs[big].height, { near: o.near, cull: o.cull, depth, face: image });
      }
      this.renderViews(ids, imgs, bufs, (i, v, s, w, h) => {
        s.rasterizer.encodeDepth(null, [depthKind, 'weight_sum']);
        rasterizer.encode(src.vertices, src.V, src.faces, src.F, null, bufs[v], w, h, { near: o.near, cull: o.cull, depth, face: image });
        visibility.accumulate(image, w, h, { meshDepth: depth, modelDepth: s.rasterizer.getDepthTextureView(depthKind),
          modelWeightSum: s.rasterizer.getDepthTextureView('weight_sum'), minWeightSum, threshold });
        totals.push(visibility.stats());
      }, () => { visibility.reset(src.F); totals.length = 0; }, what);
      dev.synchronize();
    } catch (e) {
      visibility.destroy();
      throw e;
    } finally { rasterizer.destroy(); depth.destroy(); image.destroy(); }
    return { visibility, ids, totals };
  }
  /** Which faces of `mesh` (hip.rasterizeMesh's: typed arrays or an object of HipBuffers) the views see, and where the model agrees with them: per view the
   *  mesh is rasterized under the view's camera and its face image accumulated (hip.FaceVisibility) beside the mesh's depth and the model's depthKind depth
   *  map.  options: { viewIds, split = 'train', depthKind = 'median', threshold = 0.05, minWeightSum = 0.5, near, cull }.  Returns { iteration, views,
   *  counters: Uint32Array[3 F] (pixels, agreeing, views per face), counted, agreeing, foreign (one entry per view), ms }.  hip.selectFaces turns the counters
   *  into a mask and hip.filterFaces applies it; cullMesh does both on the device.  Rendered through evaluate's passes with its isolation.  Same results as
   *  the Python host's. */
  meshVisibility(mesh, options) {
    const o = options || {}, t0 = Date.now(), src = hip.meshOnDevice(this.device, mesh, 'meshVisibility');
    let acc = null;
    try {
      acc = this.faceVisibilityOver('meshVisibility', src, o);
      return Object.assign({ iteration: this.trainer.iteration, views: acc.ids, counters: acc.visibility.read() }, perView(acc.totals), { ms: Date.now() - t0 });
    } finally {
      if (acc) acc.visibility.destroy();
      if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
    }
  }
  /** `mesh` without the faces the views do not see: meshVisibility's counters, hip.selectFaces' rule on them and hip.filterFaces, with flags and compaction on
   *  the device.  options: the rule { minPixels = 1, minViews = 1, minAgreeing = 0, minAgreeingFraction = 0 } and meshVisibility's options.  Returns
   *  filterFaces' object (colours / keys of a typed-array mesh gathered through vertexMap) with counters, the counters of the input's faces, and views added.
   *  Same results as the Python host's. */
  cullMesh(mesh, options) {
    const o = options || {}, dev = this.device;
    hip.selectFaces(new Uint32Array(0), o);   // (the rule is checked before anything is rendered)
    const src = hip.meshOnDevice(dev, mesh, 'cullMesh');
    let acc = null, keep = null, out;
    try {
      acc = this.faceVisibilityOver('cullMesh', src, o);
      keep = dev.createBuffer({ size: Math.max(src.F, 8), label: 'face keep flags' });
      acc.visibility.flags(keep, o);
      out = hip.filterFaces(dev, { vertices: src.vertices, faces: src.faces, numVertices: src.V, numFaces: src.F }, keep);
      out.counters = acc.visibility.read();
      out.views = acc.ids;
    } finally {
      if (acc) acc.visibility.destroy();
      if (keep) keep.destroy();
      if (src.own) { src.vertices.destroy(); src.faces.destroy(); }
    }
    hip.gatherVertexAttributes(mesh, out);
    return out;
  }

  // ---------------------------------------------------------------- vertex colours from the photographs (DESIGN.md section 22)
  /** `mesh` (hip.bakeVertexColours': typed arrays or an object of HipBuffers) with its vertex colours taken from the split's photographs -- the device copies
   *  the trainer holds -- under the split's cameras: hip.bakeVertexColours with its options and { viewIds, split = 'train' }, and its result with views
   *  added.  The views may differ in size.  Nothing is rendered through the model: the pipeline is drained and that is all.  Same results as the Python
   *  host's. */
  bakeMeshColours(mesh, options) {
    const o = options || {}, { imgs, bufs, ids } = this.views('bakeMeshColours', o.viewIds, o.split || 'train');
    this.drain();
    const views = ids.map((v) => ({ camera: bufs[v], image: imgs[v].texture, width: imgs[v].width, height: imgs[v].height }));
    return Object.assign(hip.bakeMeshFromViews(this.device, mesh, views, o, 'bakeMeshColours'), { views: ids });
  }

  // ---------------------------------------------------------------- a texture atlas from the photographs (DESIGN.md section 23)
  /** `mesh` with a texture atlas taken from the split's photographs under the split's cameras: hip.bakeTexture over the device copies the trainer holds, with
   *  its options and { viewIds, split = 'train' }, and its result with views added.  Nothing is rendered through the model: the pipeline is drained and that
   *  is all.  Same results as the Python host's. */
  bakeMeshTexture(mesh, options) {
    const o = options || {}, { imgs, bufs, ids } = this.views('bakeMeshTexture', o.viewIds, o.split || 'train');
    this.drain();
    const views = ids.map((v) => ({ camera: bufs[v], image: imgs[v].texture, width: imgs[v].width, height: imgs[v].height }));
    return Object.assign(hip.bakeTextureFromViews(this.device, mesh, views, o, 'bakeMeshTexture'), { views: ids });
  }

  // ---------------------------------------------------------------- TSDF fusion and mesh extraction (DESIGN.md section 13)
  /** Fuses the current model's depth maps into `volume` (hip.TSDFVolume): for each view in the order given, the forward pass, rasterize,
   *  encodeDepth([depthKind, 'weight_sum']) and volume.integrate with the weight sum and the rasterizer's output texture as colour (where the volume
   *  has colour).  Returns the view list.  Rendered through evaluate's passes with its isolation; a view is integrated only once its render is known
   *  not to have overflowed its tile-entry lists (one wait per view).  Same results as the Python host's. */
  fuseDepth(volume, viewIds, split, depthKind) {
    split = split || 'train'; depthKind = depthKind || 'median';
    if (depthKind !== 'median' && depthKind !== 'expected') throw new Error(`fuseDepth: depthKind must be 'median' or 'expected', not ${depthKind}`);
    const { imgs, bufs, ids } = this.views('fuseDepth', viewIds, split);
    this.drain();
    for (const v of ids) {
      this.renderViews([v], imgs, bufs, () => {}, null, 'fuseDepth');   // (returns with the view's complete frame in its pass set)
      const w = imgs[v].width, h = imgs[v].height, rast = this.set(w, h, bufs[v]).rasterizer;
      rast.encodeDepth(null, [depthKind, 'weight_sum']);
      volume.integrate(rast.getDepthTextureView(depthKind), bufs[v], w, h, { weightSum: rast.getDepthTextureView('weight_sum'),
        colour: volume.colour ? rast.getOutputTextureView() : null });
    }
    return ids;
  }
  /** Scores the current model's geometry against `reference` -- a Float32Array [M*3] of surface points, or the path of a PLY that holds them:
   *  extractMesh(lo, hi, voxelSize, options), hip.sampleMesh at options.density samples per unit area (default 1 / (voxelSize / 2)^2, a spacing of half a
   *  voxel; options.seed, default 0) and hip.geometryMetrics(samples, reference, maxDistance, threshold).  Returns its object -- accuracy, completeness,
   *  chamfer, precision, recall, fscore and the counts -- with vertices, faces, samples (the mesh's and the sample count) and ms.  extractMesh's isolation
   *  (fuseDepth's) and its keepLargest, minTriangles, minFraction; no alignment is attempted: the reference is taken to be in the scene's frame. */
  evaluateGeometry(reference, lo, hi, voxelSize, maxDistance, threshold, options) {
    const o = options || {}, t0 = Date.now();
    const ref = typeof reference === 'string' ? require('./loaders.js').loadPointsPLY(reference) : reference;
    const density = o.density === undefined || o.density === null ? 1.0 / (0.5 * voxelSize) ** 2 : o.density;
    const mesh = this.extractMesh(lo, hi, voxelSize, o);
    const samples = hip.sampleMesh(this.device, mesh, density, o.seed || 0, { asBuffers: true });
    let out;
    try {
      out = hip.geometryMetrics(this.device, samples.points, ref, maxDistance, threshold, { numPoints: samples.count });
    } finally { samples.points.destroy(); samples.face.destroy(); }
    return Object.assign(out, { vertices: mesh.vertices.length / 3, faces: mesh.faces.length / 3, samples: samples.count, ms: Date.now() - t0 });
  }
  /** The current model as a triangle mesh of the box [lo, hi]: TSDFVolume.fromBounds, fuseDepth over the views, extractMesh(minWeight); the volume is
   *  destroyed.  options: { viewIds, split, depthKind, minWeight, truncation, maxWeight, colour, keepLargest, minTriangles, minFraction }.  With one of the
   *  last three set the mesh goes through hip.removeSmallComponents (the floaters of a fused mesh are small components of their own) and its object is
   *  returned; otherwise the raw level set, as before, and nothing more is launched.  loaders.saveMeshPLY writes the result.
   *  options.weld: 'host' (default) or 'device' (DESIGN.md section 17): the triangles are welded where the volume emitted them and, with a component rule,
   *  labelled, selected and compacted there as well; the compacted mesh is what is read, colours and keys are read at the welded mesh's size and gathered
   *  through vertexMap.  The same bytes either way.
   *  options.simplify: a cell size (DESIGN.md section 18): the mesh is simplified last -- after welding and component removal, so that floaters are not
   *  merged into the surface first -- by hip.simplifyMesh on the grid of that cell size from the volume's lo, and its object is returned.  With weld
   *  'device' positions and faces stay on the device from the volume to the simplified mesh; with a component rule the colours alone are gathered through
   *  vertexMap on the host.  The same bytes either way; without it, as before, and nothing more is launched.
   *  options.smooth: an iteration count, and options.normals (DESIGN.md section 19): hip.smoothMesh with its defaults after welding and component removal and
   *  BEFORE simplify -- the fine mesh is denoised, then decimated -- with stats added; and normals, hip.vertexNormals of the final mesh.  With weld 'device'
   *  the positions stay on the device through both.  Without them: as before, no new key and nothing more launched. */
  extractMesh(lo, hi, voxelSize, options) {
    const o = options || {}, weld = o.weld || 'host';
    if (weld !== 'host' && weld !== 'device') throw new Error(`extractMesh: weld must be 'host' or 'device', not ${weld}`);
    const unset = (x) => x === undefined || x === null;
    if (!unset(o.texture) && o.texture !== false) {   // (DESIGN.md section 23: last of all, after bake)
      const mesh = this.extractMesh(lo, hi, voxelSize, Object.assign({}, o, { texture: null }));
      return this.bakeMeshTexture(mesh, Object.assign({ viewIds: o.viewIds, split: o.split }, o.texture === true ? {} : o.texture));
    }
    if (!unset(o.bake) && o.bake !== false) {   // (DESIGN.md section 22: last, on the final mesh; its normals are the weights even when none are asked for)
      const mesh = this.extractMesh(lo, hi, voxelSize, Object.assign({}, o, { bake: null }));
      const out = this.bakeMeshColours(mesh, Object.assign({ viewIds: o.viewIds, split: o.split }, o.bake === true ? {} : o.bake));
      out.bakeStats = out.stats;
      if (mesh.stats !== undefined) out.stats = mesh.stats; else delete out.stats;
      return out;
    }
    if (!unset(o.cull)) {   // (DESIGN.md section 21: after welding and component removal, before smooth, simplify and normals)
      const mesh = this.extractMesh(lo, hi, voxelSize, Object.assign({}, o, { cull: null, simplify: null, smooth: null, normals: false }));
      const culled = this.cullMesh(mesh, Object.assign({ viewIds: o.viewIds, split: o.split, depthKind: o.depthKind }, o.cull));
      return hip.finishMesh(this.device, culled, Float32Array.from(lo), unset(o.smooth) ? null : o.smooth, unset(o.simplify) ? null : o.simplify, !!o.normals);
    }
    const everything = unset(o.keepLargest) && !(o.minTriangles > 0) && !(o.minFraction > 0);
    const rule = { keepLargest: o.keepLargest, minTriangles: o.minTriangles, minFraction: o.minFraction };
    if (!unset(o.simplify) || !unset(o.smooth) || o.normals) return this.extractFinished(lo, hi, voxelSize, o, weld, everything, rule);
    const volume = hip.TSDFVolume.fromBounds(this.device, lo, hi, voxelSize, { truncation: o.truncation, maxWeight: o.maxWeight, colour: o.colour });
    let mesh = null, welded = null;
    try {
      this.fuseDepth(volume, o.viewIds, o.split, o.depthKind);
      if (weld === 'host' || everything) {
        mesh = volume.extractMesh(o.minWeight, { weld });
      } else {
        const tri = volume.extractTriangleBuffers(o.minWeight);
        try { welded = hip.weldTrianglesDevice(this.device, tri, { asBuffers: true }); } finally { hip.destroyBuffers(tri); }
      }
    } finally { volume.destroy(); }
    if (everything) return mesh;
    if (!welded) return hip.removeSmallComponents(this.device, mesh, rule);
    try {
      const out = hip.removeSmallComponents(this.device, { vertices: welded.vertices, faces: welded.faces }, rule);
      const V = welded.numVertices, bytes = (b, n) => (n ? this.device.readBuffer(b, n) : new ArrayBuffer(0));
      out.colours = null;
      if (welded.colours) {
        const rgba = new Uint8Array(bytes(welded.colours, 4 * V));
        out.colours = new Uint8Array(3 * out.vertexMap.length);
        out.vertexMap.forEach((old, i) => { for (let a = 0; a < 3; a++) out.colours[3 * i + a] = rgba[4 * old + a]; });
      }
      const keys = new BigUint64Array(bytes(welded.keys, 8 * V));
      out.keys = BigUint64Array.from(out.vertexMap, (old) => keys[old]);
      return out;
    } finally { hip.destroyBuffers(welded); }
  }
  /** extractMesh with options.simplify, smooth or normals set: volume, weld, component removal (when a rule is given), then hip.finishMesh: smoothing,
   *  simplification from the volume's origin, normals. */
  extractFinished(lo, hi, voxelSize, o, weld, everything, rule) {
    const unset = (x) => x === undefined || x === null;
    const simplify = unset(o.simplify) ? null : o.simplify, smooth = unset(o.smooth) ? null : o.smooth, normals = !!o.normals;
    const volume = hip.TSDFVolume.fromBounds(this.device, lo, hi, voxelSize, { truncation: o.truncation, maxWeight: o.maxWeight, colour: o.colour });
    let welded = {}, kept = {};
    try {
      this.fuseDepth(volume, o.viewIds, o.split, o.depthKind);
      const origin = volume.origin;
      if (everything) return volume.extractMesh(o.minWeight, { weld, simplify, smooth, normals });
      if (weld === 'host') {
        return hip.finishMesh(this.device, hip.removeSmallComponents(this.device, volume.extractMesh(o.minWeight), rule), origin, smooth, simplify, normals);
      }
      const tri = volume.extractTriangleBuffers(o.minWeight);
      try { welded = hip.weldTrianglesDevice(this.device, tri, { asBuffers: true }); } finally { hip.destroyBuffers(tri); }
      kept = hip.removeSmallComponents(this.device, { vertices: welded.vertices, faces: welded.faces }, Object.assign({ asBuffers: true }, rule));
      const V = welded.numVertices, nv = kept.numVertices, nf = kept.numFaces, bytes = (b, n) => (n ? this.device.readBuffer(b, n) : new ArrayBuffer(0));
      if (simplify !== null && welded.colours) {
        const all = new Uint32Array(bytes(welded.colours, 4 * V)), map = new Uint32Array(bytes(kept.vertexMap, 4 * nv));
        const gathered = Uint32Array.from(map, (old) => all[old]);
        kept.colours = this.device.createBuffer({ size: Math.max(gathered.byteLength, 8), label: 'compacted colours' });
        if (gathered.byteLength) this.device.queue.writeBuffer(kept.colours, 0, gathered);
      }
      // what removeSmallComponents returns for the typed-array mesh: colours and keys gathered through vertexMap
      const read = (device, b) => {
        const out = { vertices: new Float32Array(bytes(b.vertices, 12 * nv)), faces: new Uint32Array(bytes(b.faces, 12 * nf)),
          vertexMap: new Uint32Array(bytes(b.vertexMap, 4 * nv)), faceMap: new Uint32Array(bytes(b.faceMap, 4 * nf)), components: b.components, colours: null };
        if (welded.colours) {
          const rgba = new Uint8Array(bytes(welded.colours, 4 * V));
          out.colours = new Uint8Array(3 * nv);
          out.vertexMap.forEach((old, i) => { for (let a = 0; a < 3; a++) out.colours[3 * i + a] = rgba[4 * old + a]; });
        }
        const keys = new BigUint64Array(bytes(welded.keys, 8 * V));
        out.keys = BigUint64Array.from(out.vertexMap, (old) => keys[old]);
        return out;
      };
      return hip.finishMesh(this.device, kept, origin, smooth, simplify, normals, read);
    } finally {
      volume.destroy();
      hip.destroyBuffers(welded);
      hip.destroyBuffers(kept);
    }
  }

  // ---------------------------------------------------------------- render contribution (DESIGN.md section 11)
  /** { stats, ids }: the views' contribution records accumulated into one new device buffer (Trainer.pruneByContribution decides on it). */
  contributionBuffer(viewIds, split, what) {
    const { imgs, bufs, ids } = this.views(what, viewIds, split);
    if (ids.reduce((a, v) => a + imgs[v].width * imgs[v].height, 0) >= 2 ** 32) throw new RangeError(`${what}: the views hold 2^32 pixels or more; the per-Gaussian pixel count is 32 bits wide`);
    this.drain();
    const stats = hip.createContributionBuffer(this.device, this.trainer.pointCloud.num_points);
    try {
      this.renderViews(ids, imgs, bufs, (i, v, s) => s.rasterizer.encodeContribution(null, stats), () => hip.addon.bufferClear(this.device.handle, stats.ptr, stats.size), what);
    } catch (e) { stats.destroy(); throw e; }
    return { stats, ids };
  }
  /** How much of each Gaussian the views' images hold: { sum_q, weight_sum, max_weight, pixels, views }, one entry per Gaussian, accumulated over
   *  the views (default: all training views).  Rendered through evaluate's passes with its isolation (drained pipeline, overflow-and-regrow with the
   *  records cleared and every view walked again, no random draw, no training pass, no recording dropped).  Same results as the Python host's. */
  contributionStats(viewIds, split) {
    const { stats, ids } = this.contributionBuffer(viewIds, split || 'train', 'contributionStats');
    try { return Object.assign(hip.readContribution(stats, this.trainer.pointCloud.num_points), { views: ids }); } finally { stats.destroy(); }
  }
}

exports.Evaluator = Evaluator;   // (assigned, not replaced: trainer.js and this module require each other)
