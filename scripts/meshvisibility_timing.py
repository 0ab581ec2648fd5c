#!/usr/bin/env python3
"""Per-face visibility and the face filter on the device: per-kernel times on the meshes of scripts/meshraster_timing.py and on crafted face images.

    python scripts/meshvisibility_timing.py [--out profiles/meshvisibility_timing.json]    (needs an MI355X)

Meshes: the latitude-longitude sphere of 3.92 M faces (the size of a 512^3 fusion's mesh) and ops.simplifyMesh of it at cells of 2 "voxels" of 8 / 512 (the size
of a 256^3 one), rasterized into 1920 x 1080.  Per mesh, medians of five of the library's event-bracketed kernel times, in microseconds:
  encode       MeshRasterizer.encode with the depth and the face image: the yardstick, the work that feeds one accumulate;
  accumulate   FaceVisibility.accumulate of that face image alone (4 bytes per pixel read) and with the mesh's depth as both depth images and a weight sum
               (16 bytes per pixel read);
  flags        FaceVisibility.flags: the pack of the counters and the rule (12 + 12 + 16 + 1 bytes per face);
  select       MeshFaceFilter.select under those flags: the flag kernel and the library's two scans;
  compact      MeshFaceFilter.compact with positions and both maps.
Crafted face images at 1920 x 1080 -- one face on every pixel, two faces alternating per pixel, uniform random faces among 3.9 M -- give accumulate's bounds: one
address and the longest runs, two addresses and no run at all, no two neighbours equal over a table far larger than the caches.  bytes over time is set against
the 6.1 TB/s that consecutive 16-byte elements stream at on the same box.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from meshraster_timing import kernel_times, sphere, upload, wall   # noqa: E402

RASTER = ("raster_vertices", "raster_faces", "raster_blocks", "raster_resolve", "scan_reduce", "scan_block_sums", "scan_downsweep")
ACCUMULATE = ("face_visibility_accumulate", "face_visibility_advance")
FLAGS = ("face_visibility_pack", "face_visibility_flags")
SELECT = ("face_filter_flags", "scan_reduce", "scan_block_sums", "scan_downsweep")
COMPACT = ("mesh_emit_vertices", "mesh_emit_faces")


def timed(dev, fn, names, nbytes=None):
    fn()
    out = dict(kernel_times(dev, fn, names=names), host_clock_ms=wall(dev, fn)["ms_median"])
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["GBps"] = nbytes / out["sum_us"] / 1e3
    return out


def measure_mesh(dev, ops, name, mesh, cam, W, H):
    V, F, npix = mesh["numVertices"], mesh["numFaces"], W * H
    rasterizer, visibility, filt = ops.MeshRasterizer(dev), ops.FaceVisibility(dev), ops.MeshFaceFilter(dev)
    depth, face, keep = dev.createBuffer(4 * npix), dev.createBuffer(4 * npix), dev.createBuffer(max(F, 1))
    outs = []
    try:
        out = dict(vertices=V, faces=F, width=W, height=H)
        out["encode"] = timed(dev, lambda: rasterizer.encode(mesh["vertices"], V, mesh["faces"], F, None, cam, W, H, depth=depth, face=face), RASTER)
        out["stats"] = rasterizer.stats()
        visibility.reset(F)
        out["accumulate, face image"] = timed(dev, lambda: visibility.accumulate(face, W, H), ACCUMULATE, 4 * npix)
        out["accumulate, depths and weight sum"] = timed(dev, lambda: visibility.accumulate(face, W, H, depth, depth, depth, 0.5, 0.05), ACCUMULATE, 16 * npix)
        out["visibility"] = visibility.stats()
        out["flags"] = timed(dev, lambda: visibility.flags(keep), FLAGS, 41 * F)
        counters = visibility.read()
        out["faces_seen"] = int((counters[:, 0] > 0).sum())
        out["select"] = timed(dev, lambda: filt.select(mesh["faces"], F, V, keep), SELECT)
        kv, kf, _ = filt.select(mesh["faces"], F, V, keep)
        outs = [dev.createBuffer(s * max(n, 1)) for s, n in ((12, kv), (12, kf), (4, kv), (4, kf))]
        out["compact"] = timed(dev, lambda: filt.compact(mesh["vertices"], *outs), COMPACT)
        out["kept"] = dict(vertices=kv, faces=kf)
    finally:
        for o in [rasterizer, visibility, filt, depth, face, keep] + outs:
            o.destroy()
    print(name, json.dumps(out), flush=True)
    return out


def measure_image(dev, ops, name, img, F, W, H):
    visibility = ops.FaceVisibility(dev)
    buf = dev.bufferFrom(img)
    try:
        visibility.reset(F)
        out = dict(faces=F, width=W, height=H, **timed(dev, lambda: visibility.accumulate(buf, W, H), ACCUMULATE, 4 * W * H))
        out["visibility"] = visibility.stats()
    finally:
        visibility.destroy()
        buf.destroy()
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshvisibility_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import ops, synth
    dev = ops.HipDevice(0)
    W, H = 1920, 1080
    result = dict(note="kernel times: the library's event-bracketed launches of one call, per kernel the median of five, in microseconds; host-clock times in ms, each "
                       "call followed by a wait; GBps: the bytes that must move over the sum of the kernel times")
    v, f, col = sphere()
    fine = upload(dev, v, f, col)
    cam = dev.bufferFrom(synth.camera_block(np.eye(4), W, H, H / 0.9))
    coarse = ops.simplifyMesh(dev, fine, 2 * 8.0 / 512, origin=(-4.0, -4.0, 4.0), asBuffers=True)
    result["meshes"] = {}
    for name, m in (("sphere, 3.92 M faces", fine), ("simplify 2 voxels", coarse)):
        result["meshes"][name] = measure_mesh(dev, ops, name, m, cam, W, H)
    for m in (fine, coarse):
        ops.destroyBuffers({k: b for k, b in m.items() if isinstance(b, ops.HipBuffer)})
    cam.destroy()
    rng = np.random.default_rng(1)
    F = 3920000
    result["images"] = {}
    for name, img in (("one face on every pixel", np.full(W * H, 12345, np.uint32)), ("two faces alternating per pixel", (np.arange(W * H) % 2).astype(np.uint32) * 7 + 3),
                      ("uniform random faces among 3.9 M", rng.integers(0, F, W * H).astype(np.uint32))):
        result["images"][name] = measure_image(dev, ops, name, img, F, W, H)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
