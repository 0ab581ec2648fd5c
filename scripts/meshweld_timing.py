#!/usr/bin/env python3
"""Welding on the device against welding on the host: per-kernel times, passes and host-clock times on fused TSDF meshes and on the sort's adversarial shapes.

    python scripts/meshweld_timing.py [--sizes 256,512] [--views 8] [--adversarial 12000000] [--out profiles/meshweld_timing.json]    (needs an MI355X)

The meshes are those of scripts/tsdf_timing.py: the c2 scene (100 000 Gaussians, 640 x 480) rendered from cameras on a circle, its median depth fused
into a cube of 256^3 and of 512^3 voxels.  The volume emits its triangles into device buffers once; from there, in one process,
  device: ops.weldTrianglesDevice on the buffers, read-back of the V- and F-sized result included, by the host's clock (median of five), and per kernel
          the median of the library's event-bracketed times over five count + emit calls, with the passes that ran;
  host:   today's path, the read-back of the soup (positions, keys, colours) and ops.weldTriangles (np.unique), by the host's clock (median of three).
The two results are compared byte for byte.  The adversarial shapes -- all keys equal, keys that differ only in the top byte, uniformly random u64 (all
eight passes run) -- are welded the same way at --adversarial slots, with zero positions.  bytes_per_pass is what one pass must move (a histogram read of
the keys, a scatter's read and write of the pairs: 8 + 12 + 12 bytes per slot), to set against the hbm_stream rate in profiles/.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("weld_key_bits", "weld_plan", "weld_histogram", "scan_reduce", "scan_block_sums", "scan_downsweep", "weld_scatter", "weld_heads", "weld_emit")
PASS_BYTES_PER_SLOT = 8 + 12 + 12


def wall(fn, runs):
    out, result = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        result = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return result, dict(ms_median=float(np.median(out)), ms_runs=out)


def measure(dev, ops, name, tri, host=True):
    """tri: dict(positions, keys, colours | None as HipBuffer, numTriangles)."""
    F = tri["numTriangles"]
    S = 3 * F
    out = dict(triangles=F, slots=S)
    welder = ops.MeshWelder(dev)
    try:
        V = welder.count(tri["keys"], S)
        outs = [dev.createBuffer(n) for n in (4 * S, 12 * V, 4 * V, 8 * V)]
        cols = tri["colours"]

        def kernels():
            welder.count(tri["keys"], S)
            welder.emit(tri["keys"], S, tri["positions"], cols, outs[0], outs[1], outs[2] if cols is not None else None, outs[3], V)

        kernels()
        dev.synchronize()
        per = {k: [] for k in KERNELS}
        launches = {}
        for _ in range(5):
            dev.kernelTimes(reset=True)
            dev.setProfiling(True)
            kernels()
            dev.synchronize()
            dev.setProfiling(False)
            kt = dev.kernelTimes(reset=True)
            for k in KERNELS:
                per[k].append(1e3 * kt.get(k, (0, 0.0))[1])
                launches[k] = kt.get(k, (0, 0.0))[0]
        med = {k: float(np.median(v)) for k, v in per.items()}
        stats = welder.stats()
        out.update(vertices=V, passes_run=stats["passesRun"], passes_skipped=stats["passesSkipped"], kernels_us_median=med, kernels_us_runs=per, launches=launches,
                   kernels_sum_us=float(sum(med.values())), bytes_per_pass=PASS_BYTES_PER_SLOT * S)
        if stats["passesRun"]:
            # the histogram and scatter launches of skipped passes return at once; what is left per pass that ran
            out["pass_us"] = (med["weld_histogram"] + med["weld_scatter"]) / stats["passesRun"]
            out["pass_GBps"] = out["bytes_per_pass"] / out["pass_us"] / 1e3
        for b in outs:
            b.destroy()
    finally:
        welder.destroy()
    device_mesh, out["device_weld_with_readback"] = wall(lambda: ops.weldTrianglesDevice(dev, tri), 5)
    if host:
        def today():
            soup = dict(positions=tri["positions"].read(np.float32, count=3 * S).reshape(F, 3, 3), keys=tri["keys"].read(np.uint64, count=S).reshape(F, 3),
                        colours=tri["colours"].read(np.uint8, count=4 * S).reshape(F, 3, 4) if tri["colours"] is not None else None)
            t1 = time.perf_counter()
            mesh = ops.weldTriangles(soup)
            today.unique_ms.append((time.perf_counter() - t1) * 1e3)
            return mesh
        today.unique_ms = []
        host_mesh, out["host_readback_and_weld"] = wall(today, 3)
        out["host_readback_and_weld"]["np_unique_ms_median"] = float(np.median(today.unique_ms))
        out["equal_to_host"] = bool(all((host_mesh[k] is None and device_mesh[k] is None) or
                                        np.array_equal(np.ascontiguousarray(host_mesh[k]).view(np.uint8), np.ascontiguousarray(device_mesh[k]).view(np.uint8))
                                        for k in ("vertices", "faces", "colours", "keys")))
    print(name, json.dumps({k: v for k, v in out.items() if k not in ("kernels_us_runs",)}), flush=True)
    return out


def fused_volumes(dev, ops, sizes, n_views):
    from webdgs_amd import synth
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
        v = dict(camera=dev.bufferFrom(c), depth=dev.createBuffer(4 * px), ws=dev.createBuffer(4 * px))
        enc.copyBufferToBuffer(rast.getDepthTextureView("median"), 0, v["depth"], 0, 4 * px)
        enc.copyBufferToBuffer(rast.getDepthTextureView("weight_sum"), 0, v["ws"], 0, 4 * px)
        dev.synchronize()
        views.append(v)
    fwd.check()
    for size in sizes:
        vol = ops.TSDFVolume(dev, (-4.0, -4.0, 2.0), 8.0 / size, (size, size, size), maxWeight=1e9, colour=False)
        for v in views:
            vol.integrate(v["depth"], v["camera"], cfg.width, cfg.height, weightSum=v["ws"])
        tri = vol.extractTriangleBuffers()
        vol.destroy()
        yield size, tri
        ops.destroyBuffers(tri)
    rast.destroy()
    fwd.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--adversarial", type=int, default=12000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshweld_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import ops
    dev = ops.HipDevice(0)
    result = dict(note="kernel times: the library's event-bracketed launches of one count + emit, per kernel the median of five calls (all eight passes' histogram and "
                       "scatter launches, those of skipped passes returning at once; nine scans: eight digit tables and the head flags); host-clock times in ms",
                  tsdf={}, adversarial={})
    for size, tri in fused_volumes(dev, ops, [int(s) for s in args.sizes.split(",") if s], args.views):
        result["tsdf"][str(size)] = measure(dev, ops, f"tsdf {size}^3", tri)
    n = args.adversarial // 3 * 3
    if n:
        rng = np.random.default_rng(17)
        shapes = (("all-equal", np.full(n, 0x0123456789ABCDEF, np.uint64)),
                  ("top-byte-only", np.uint64(0x00C0FFEE12345678) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56))),
                  ("random-u64", rng.integers(0, 2 ** 64, n, dtype=np.uint64)))
        for name, keys in shapes:
            tri = dict(keys=dev.bufferFrom(keys), positions=dev.createBuffer(12 * n), colours=None, numTriangles=n // 3)
            result["adversarial"][name] = measure(dev, ops, f"{name} {n}", tri)
            ops.destroyBuffers(tri)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
