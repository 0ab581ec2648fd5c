#!/usr/bin/env python3
"""Mesh connected components and small-component removal: per-kernel times on fused TSDF meshes and on the union-find's adversarial shapes.

    python scripts/meshclean_timing.py [--sizes 256,512] [--views 8] [--adversarial 4000000] [--out profiles/meshclean_timing.json]    (needs an MI355X)

The meshes are those of scripts/tsdf_timing.py: the c2 scene (100 000 Gaussians, 640 x 480) rendered from cameras on a circle, its median depth fused
into a cube of 256^3 and of 512^3 voxels, extracted and welded.  Each mesh is uploaded once and, device-resident, labelled (MeshComponents.label) and
reduced to its largest component (select + compact) five times; per kernel the median of the library's event-bracketed times over the five runs is
kept, and their sum.  The host restatement (tests/meshclean_ref.py) labels the same mesh once, by wall clock: what a user saves by staying on the
device.  The adversarial shapes -- a strip numbered against the thread order, which builds the deepest trees, and a star, where every union contends
on one root -- are labelled the same way at --adversarial faces.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LABEL_KERNELS = ("mesh_init", "mesh_hook", "mesh_flatten", "mesh_mark", "scan_reduce", "scan_block_sums", "scan_downsweep", "mesh_label_vertices", "mesh_label_faces")
COMPACT_KERNELS = ("mesh_keep_flags", "scan_reduce", "scan_block_sums", "scan_downsweep", "mesh_emit_vertices", "mesh_emit_faces")


def timed(dev, fn, names, runs=5):
    """Per kernel name the median over `runs` of the summed event times of one call of fn (us), their sum, and the call's wall-clock median (ms)."""
    fn()
    dev.synchronize()
    per, wall = {k: [] for k in names}, []
    for _ in range(runs):
        dev.kernelTimes(reset=True)
        dev.setProfiling(True)
        t0 = time.perf_counter()
        fn()
        dev.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.setProfiling(False)
        kt = dev.kernelTimes(reset=True)
        for k in names:
            per[k].append(1e3 * kt.get(k, (0, 0.0))[1])
    med = {k: float(np.median(v)) for k, v in per.items()}
    return dict(kernels_us_median=med, kernels_us_runs=per, sum_us=float(sum(med.values())), wall_ms_median=float(np.median(wall)), wall_ms_runs=wall)


def measure(dev, ops, name, vertices, faces, restate):
    import meshclean_ref as M
    V, F = vertices.shape[0], faces.shape[0]
    vbuf, fbuf = dev.bufferFrom(vertices), dev.bufferFrom(faces)
    comp = ops.MeshComponents(dev)
    out = dict(vertices=V, faces=F)
    try:
        out["label"] = timed(dev, lambda: comp.label(fbuf, F, V), LABEL_KERNELS)
        labels = comp.read()
        sizes = labels["triangles"]
        out.update(components=int(labels["count"]), invalid_faces=int(labels["invalidFaces"]), largest=int(sizes.max()) if sizes.size else 0,
                   singletons=int(np.sum(sizes == 1)))
        keep = ops.selectComponents(sizes, keepLargest=1)
        kv, kf = comp.select(keep)
        bufs = [dev.createBuffer(s * max(n, 1)) for s, n in ((12, kv), (12, kf), (4, kv), (4, kf))]

        def compact():
            comp.select(keep)
            comp.compact(vbuf, bufs[0], bufs[1], bufs[2], bufs[3], kv, kf)

        out["keep_largest"] = dict(kept_vertices=kv, kept_faces=kf, **timed(dev, compact, COMPACT_KERNELS))
        for b in bufs:
            b.destroy()
        if restate:
            t0 = time.perf_counter()
            ref = M.components(faces, V)
            out["host_restatement_label_s"] = time.perf_counter() - t0
            out["equal_to_restatement"] = bool(all(np.array_equal(labels[k], ref[k]) for k in ("faceComponent", "vertexComponent", "triangles", "vertices")))
    finally:
        comp.destroy()
    print(name, json.dumps({k: v for k, v in out.items() if k not in ("label", "keep_largest")}), "label us", round(out["label"]["sum_us"], 1),
          json.dumps({k: round(v, 1) for k, v in out["label"]["kernels_us_median"].items()}), "keep-largest us", round(out["keep_largest"]["sum_us"], 1), flush=True)
    return out


def fused_meshes(dev, ops, sizes, n_views):
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
        t0 = time.perf_counter()
        mesh = vol.extractMesh()
        print(f"{size}^3: extracted and welded in {time.perf_counter() - t0:.1f} s", flush=True)
        vol.destroy()
        yield size, mesh
    rast.destroy()
    fwd.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--adversarial", type=int, default=4000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshclean_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import ops
    import meshclean_ref as M
    dev = ops.HipDevice(0)
    result = dict(runs=5, note="kernel times: the library's event-bracketed launches, per kernel the median of five calls; the scan kernels run once per label and "
                                "twice per select", tsdf={}, adversarial={})
    for size, mesh in fused_meshes(dev, ops, [int(s) for s in args.sizes.split(",") if s], args.views):
        result["tsdf"][str(size)] = measure(dev, ops, f"tsdf {size}^3", mesh["vertices"], mesh["faces"], restate=True)
    n = args.adversarial
    if n:
        for name, (faces, V) in (("chain-descending", M.chain(n, "descending")), ("chain-ascending", M.chain(n, "ascending")), ("star-low-hub", M.star(n, "lowest")),
                                 ("star-high-hub", M.star(n, "highest"))):
            result["adversarial"][name] = measure(dev, ops, f"{name} {n}", np.zeros((V, 3), np.float32), faces, restate=False)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
