#!/usr/bin/env python3
"""TSDF fusion and mesh extraction timing: tsdf_integrate per view, and count + scan + emit on the fused volume, at 256^3 and 512^3 voxels.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/tsdf_timing.py [sizes] [views] [stream TB/s]
                                                                                      (default: 256,512 8 6.1; needs an MI355X)

The c2 scene (100 000 Gaussians, 640 x 480) is rendered from `views` cameras on a circle; each view's median depth, weight sum and colour are copied
aside, then fused into a cube of the scene's box (z in [2, 10]) with and without colour.  The yardstick for integrate is the bytes it MUST move -- tsdf
and weight (and the three colour planes) of the voxels it updates, read and written: 16 B (40 B) per updated voxel -- over the streaming read + write
bandwidth scripts/microbench/hbm_stream.hip reaches on the same box (third argument).  The number of updates is the sum of the weights after the
fusion (max_weight is out of reach).  Times are the library's own event-bracketed kernel times; under rocprofv3 the profiler's kernel statistics hold
the same launches.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_us(kt, name):
    n, ms = kt.get(name, (0, 0.0))
    return n, 1e3 * ms


def main():
    from webdgs_amd import ops, synth
    sizes = [int(s) for s in (sys.argv[1] if len(sys.argv) > 1 else "256,512").split(",")]
    n_views = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    stream_tbs = float(sys.argv[3]) if len(sys.argv) > 3 else 6.1
    dev = ops.HipDevice(0)
    cfg = synth.CONFIGS["c2"]
    g, sh = synth.make_gaussians(cfg)
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    cams = synth.circle_cameras(cfg, n_views)
    cam = dev.bufferFrom(cams[0])
    fwd = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fwd, format="rgba8unorm"))
    px = cfg.width * cfg.height
    views = []
    enc = dev.createCommandEncoder()
    for c in cams:
        cam.write(c)
        fwd.encode(None)
        rast.encode(None, cfg.width, cfg.height)
        rast.encodeDepth(None, ("median", "weight_sum"))
        v = dict(camera=dev.bufferFrom(c), depth=dev.createBuffer(4 * px), ws=dev.createBuffer(4 * px), colour=dev.createBuffer(4 * px))
        enc.copyBufferToBuffer(rast.getDepthTextureView("median"), 0, v["depth"], 0, 4 * px)
        enc.copyBufferToBuffer(rast.getDepthTextureView("weight_sum"), 0, v["ws"], 0, 4 * px)
        enc.copyBufferToBuffer(rast.getOutputTextureView(), 0, v["colour"], 0, 4 * px)
        dev.synchronize()
        views.append(v)
    fwd.check()
    print(f"c2: {cfg.num_points} Gaussians, {cfg.width}x{cfg.height} median depth, {n_views} views; streaming read + write yardstick {stream_tbs} TB/s", flush=True)
    for size in sizes:
        for colour in (False, True):
            vol = ops.TSDFVolume(dev, (-4.0, -4.0, 2.0), 8.0 / size, (size, size, size), maxWeight=1e9, colour=colour)

            def fuse():
                for v in views:
                    vol.integrate(v["depth"], v["camera"], cfg.width, cfg.height, weightSum=v["ws"], colour=v["colour"] if colour else None)

            fuse()                      # warm: first touch of the arrays
            vol.reset()
            dev.synchronize()
            dev.kernelTimes(reset=True)
            dev.setProfiling(True)
            fuse()
            dev.synchronize()
            dev.setProfiling(False)
            n, us = kernel_us(dev.kernelTimes(reset=True), "tsdf_integrate")
            updates = float(vol.getWeightBuffer().read(np.float32).astype(np.float64).sum())
            per_voxel = 40 if colour else 16
            gbs = updates * per_voxel / (us * 1e-6) / 1e9
            print(f"{size}^3 {'with' if colour else 'without'} colour: tsdf_integrate {us / max(n, 1):.1f} us per view ({n} views, {us:.1f} us); "
                  f"{updates / max(n, 1) / size ** 3:.2%} of the voxels updated per view, {updates * per_voxel / 1e6:.1f} MB must move: {gbs:.0f} GB/s = "
                  f"{gbs / (1e3 * stream_tbs):.3f} of the yardstick; all {size ** 3 / 1e6:.0f} M voxels visited in {us / max(n, 1):.1f} us = "
                  f"{size ** 3 * max(n, 1) / (us * 1e-6) / 1e9:.1f} G voxels/s", flush=True)
            # extraction on the fused volume
            total = vol.countTriangles()
            pos = dev.createBuffer(36 * max(total, 1))
            keys = dev.createBuffer(24 * max(total, 1))
            cols = dev.createBuffer(12 * max(total, 1)) if colour else None
            emit = lambda: ops.check(dev.lib.wdgs_tsdf_volume_emit_triangles(vol.handle, pos.ptr, keys.ptr, cols.ptr if cols is not None else None, total))   # noqa: E731
            emit()
            dev.synchronize()
            dev.kernelTimes(reset=True)
            dev.setProfiling(True)
            for _ in range(5):
                vol.countTriangles()
                emit()
            dev.synchronize()
            dev.setProfiling(False)
            kt = dev.kernelTimes(reset=True)
            parts = {k: kernel_us(kt, k) for k in ("tsdf_count", "scan_reduce", "scan_block_sums", "scan_downsweep", "tsdf_emit")}
            line = ", ".join(f"{k} {u / max(c, 1):.1f}" for k, (c, u) in parts.items())
            print(f"{size}^3 {'with' if colour else 'without'} colour: {total} triangles; per extraction (us): {line}; "
                  f"count + scan + emit {sum(u / max(c, 1) for c, u in parts.values()):.1f} us", flush=True)
            for b in (pos, keys, cols):
                if b is not None:
                    b.destroy()
            vol.destroy()
    rast.destroy()
    fwd.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
