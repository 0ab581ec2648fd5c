#!/usr/bin/env python3
"""Mesh accuracy metrics timing: surface sampling, the point index's build and nearest-point queries at a million points a side.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/geometry_timing.py [samples] [volume] [views] [G wave-instr/s]
                                                                                      (default: 1000000 256 8 950; needs an MI355X)

The c2 scene (100 000 Gaussians, 640 x 480) is fused from `views` cameras into a cube of `volume`^3 voxels of the scene's box and its mesh extracted
(Trainer.extractMesh's path by hand).  The mesh is sampled twice with different seeds at the density that gives about `samples` points: one set is
indexed, the other queries it, at a cutoff of 2 and of 8 voxels -- the two directions of geometryMetrics on a surface against itself.  Reported: the
sampling kernels, the build (bounds, cells, scan, scatter), and per query the ordering kernels and `nearest`, with queries per second and the mean
number of (query, point) pairs examined, counted in a separate untimed call.  The yardstick for `nearest` is the vector-instruction rate
scripts/microbench/valu_issue.hip reaches on the same box (fourth argument, in G wave-instructions per second): a wave tests 64 pairs per trip of its
inner loop.  Times are the library's own event-bracketed kernel times; under rocprofv3 the profiler's kernel statistics hold the same launches.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIR_INSTRUCTIONS = 17   # vector instructions per pair in the gfx950 code of scan_records, unrolled by four: 3 v_sub, 3 v_mul, 2 v_add, 3 v_cmp, 2 v_cndmask, and a quarter of the 15 of addressing and loop control


def kernel_us(kt, name):
    n, ms = kt.get(name, (0, 0.0))
    return n, 1e3 * ms


def profiled(dev, fn, repeat=1):
    dev.synchronize()
    dev.kernelTimes(reset=True)
    dev.setProfiling(True)
    for _ in range(repeat):
        fn()
    dev.synchronize()
    dev.setProfiling(False)
    return dev.kernelTimes(reset=True)


def main():
    from webdgs_amd import ops, synth
    want = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    n_views = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    valu_g = float(sys.argv[4]) if len(sys.argv) > 4 else 950.0
    dev = ops.HipDevice(0)
    cfg = synth.CONFIGS["c2"]
    g, sh = synth.make_gaussians(cfg)
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    cams = synth.circle_cameras(cfg, n_views)
    cam = dev.bufferFrom(cams[0])
    fwd = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fwd, format="rgba8unorm"))
    voxel = 8.0 / size
    vol = ops.TSDFVolume(dev, (-4.0, -4.0, 2.0), voxel, (size, size, size), colour=False)
    for c in cams:
        cam.write(c)
        fwd.encode(None)
        rast.encode(None, cfg.width, cfg.height)
        rast.encodeDepth(None, ("median", "weight_sum"))
        vol.integrate(rast.getDepthTextureView("median"), cam, cfg.width, cfg.height, weightSum=rast.getDepthTextureView("weight_sum"))
        dev.synchronize()
    fwd.check()
    mesh = vol.extractMesh()
    vol.destroy()
    v, f = mesh["vertices"], mesh["faces"]
    tri = v[f.astype(np.int64)].astype(np.float64)
    area = float(0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum())
    density = want / area
    print(f"c2: {cfg.num_points} Gaussians fused from {n_views} views into {size}^3 voxels of {voxel:.5f}: {v.shape[0]} vertices, {f.shape[0]} triangles, area {area:.2f}; "
          f"density {density:.1f} per unit area; yardstick {valu_g:.0f} G wave-instructions/s", flush=True)

    # ---- sampling
    vb, fb = dev.bufferFrom(v), dev.bufferFrom(f)
    sampler = ops.MeshSampler(dev)
    sets = []
    for seed in (1, 2):
        total = sampler.count(vb, v.shape[0], fb, f.shape[0], density, seed)
        points = dev.createBuffer(12 * total)
        face = dev.createBuffer(4 * total)
        sampler.emit(vb, v.shape[0], fb, f.shape[0], density, seed, points, face)     # warm
        kt = profiled(dev, lambda: (sampler.count(vb, v.shape[0], fb, f.shape[0], density, seed), sampler.emit(vb, v.shape[0], fb, f.shape[0], density, seed, points, face)), 5)
        parts = {k: kernel_us(kt, k) for k in ("sample_count", "scan_reduce", "scan_block_sums", "scan_downsweep", "sample_emit")}
        line = ", ".join(f"{k} {u / max(c, 1):.1f}" for k, (c, u) in parts.items())
        emit_us = parts["sample_emit"][1] / max(parts["sample_emit"][0], 1)
        print(f"sampling, seed {seed}: {total} samples of {f.shape[0]} triangles; per call (us): {line}; emit {total / emit_us:.0f} M samples/s, "
              f"{16 * total / emit_us / 1e3:.0f} GB/s written", flush=True)
        face.destroy()
        sets.append((points, total))
    sampler.destroy()
    (ref, m), (qry, k) = sets

    # ---- index build and queries
    d2, idx, pairs = dev.createBuffer(4 * k), dev.createBuffer(4 * k), dev.createBuffer(8)
    for voxels in (2, 8):
        cutoff = voxels * voxel
        index = ops.PointIndex(dev, ref, count=m)
        index.nearestInto(None, qry, k, cutoff, d2, idx)      # the first query completes the build (the default cell edge); warm
        info = index.info()
        index.destroy()
        built = []

        def build():
            built.append(ops.PointIndex(dev, ref, cellSize=info["cellSize"], count=m))

        kt = profiled(dev, build, 3)
        parts = {n: kernel_us(kt, n) for n in ("point_bounds", "point_cell", "scan_reduce", "scan_block_sums", "scan_downsweep", "point_scatter")}
        line = ", ".join(f"{n} {u / max(c, 1):.1f}" for n, (c, u) in parts.items())
        print(f"cutoff {voxels} voxels = {cutoff:.4f}: index of {info['indexed']} points, cell edge {info['cellSize']:.5f} ({info['cellSize'] / voxel:.2f} voxels), grid {info['dims']}; "
              f"build per call (us): {line}; {sum(u / max(c, 1) for c, u in parts.values()):.1f} us in kernels", flush=True)
        index = built.pop()
        for b in built:
            b.destroy()
        kt = profiled(dev, lambda: index.nearestInto(None, qry, k, cutoff, d2, idx), 5)
        parts = {n: kernel_us(kt, n) for n in ("query_cell", "scan_reduce", "scan_block_sums", "scan_downsweep", "query_order", "nearest")}
        line = ", ".join(f"{n} {u / max(c, 1):.1f}" for n, (c, u) in parts.items())
        near_us = parts["nearest"][1] / max(parts["nearest"][0], 1)
        all_us = sum(u / max(c, 1) for c, u in parts.values())
        pairs.clear()
        index.nearestInto(None, qry, k, cutoff, d2, idx, pairs)
        examined = int(pairs.read(np.uint64, count=1)[0])
        stats = ops.pointDistanceStats(dev, d2, cutoff, cutoff, count=k)
        rate = examined / (near_us * 1e-6)
        ceiling = valu_g * 1e9 * 64 / PAIR_INSTRUCTIONS
        print(f"cutoff {voxels} voxels: {k} queries; per call (us): {line}; {all_us:.1f} us in kernels = {k / all_us:.1f} M queries/s ({k / near_us:.1f} M/s in nearest alone); "
              f"{examined / k:.1f} pairs examined per query, {rate / 1e9:.1f} G pair tests/s = {rate / ceiling:.3f} of {ceiling / 1e9:.0f} G "
              f"({PAIR_INSTRUCTIONS} instructions per 64 pairs at the yardstick); found {stats['n_found']} ({stats['n_found'] / k:.1%}), mean distance "
              f"{stats['mean'] / voxel:.3f} voxels", flush=True)
        # the same cutoff with a cell edge of the cutoff itself: the search without a choice of edge
        coarse = ops.PointIndex(dev, ref, cellSize=cutoff, count=m)
        coarse.nearestInto(None, qry, k, cutoff, d2, idx)
        kt = profiled(dev, lambda: coarse.nearestInto(None, qry, k, cutoff, d2, idx), 2)
        c_us = kernel_us(kt, "nearest")
        pairs.clear()
        coarse.nearestInto(None, qry, k, cutoff, d2, idx, pairs)
        c_examined = int(pairs.read(np.uint64, count=1)[0])
        print(f"cutoff {voxels} voxels, cell edge = cutoff (grid {coarse.info()['dims']}): nearest {c_us[1] / max(c_us[0], 1):.1f} us, {c_examined / k:.1f} pairs per query, "
              f"{c_examined / (c_us[1] / max(c_us[0], 1) * 1e-6) / 1e9:.1f} G pair tests/s", flush=True)
        coarse.destroy()
        index.destroy()
    rast.destroy()
    fwd.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
