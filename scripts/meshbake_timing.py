#!/usr/bin/env python3
"""Vertex-colour baking on the device: per-kernel times on the meshes of scripts/meshraster_timing.py.

    python scripts/meshbake_timing.py [--label lazy] [--out profiles/meshbake_timing.json]    (needs an MI355X)

Meshes: the latitude-longitude sphere of 3.92 M faces (1.96 M vertices) and ops.simplifyMesh of it at cells of 2 "voxels" of 8 / 512, under the camera of
scripts/meshvisibility_timing.py at 1920 x 1080, with a noise photograph.  Per mesh, medians of five of the library's event-bracketed kernel times, in
microseconds:
  encode       MeshRasterizer.encode with the depth image: the yardstick, the work that feeds one accumulate;
  accumulate   MeshColourBaker.accumulate in its four forms (with and without the depth image, with and without normals);
  resolve      MeshColourBaker.resolve with a fallback and a mask;
  shuffled     accumulate with depth and normals over the same vertices in random order: gathers without locality.
bound_us is the time the bytes that must move would take at the 6.1 TB/s that consecutive 16-byte elements stream at on the same box:
12 bytes per vertex, 12 more with normals, and 36 read and 36 written per vertex that reaches its row; the texels are not counted.
A run with --label writes into its own section of the file, so that two builds of the library (WDGS_LIB_PATH) can be set side by side: the committed file
holds the kept kernel ("lazy") beside the build that issued the colour loads in front of the depth test ("eager").
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
STREAM_BYTES_PER_US = 6.1e6


def timed(dev, fn, names):
    fn()
    return dict(kernel_times(dev, fn, names=names), host_clock_ms=wall(dev, fn)["ms_median"])


def measure_mesh(dev, ops, name, mesh, normals, cam, image, W, H, shuffled=None):
    V, F, npix = mesh["numVertices"], mesh["numFaces"], W * H
    rasterizer, baker = ops.MeshRasterizer(dev), ops.MeshColourBaker(dev)
    depth, colours, mask = dev.createBuffer(4 * npix), dev.createBuffer(4 * max(V, 1)), dev.createBuffer(max(V, 1))
    try:
        out = dict(vertices=V, faces=F, width=W, height=H)
        out["encode"] = timed(dev, lambda: rasterizer.encode(mesh["vertices"], V, mesh["faces"], F, None, cam, W, H, depth=depth), RASTER)
        forms = [("depth and normals", mesh["vertices"], normals, depth), ("depth", mesh["vertices"], None, depth), ("normals", mesh["vertices"], normals, None),
                 ("neither", mesh["vertices"], None, None)]
        if shuffled is not None:
            forms.append(("depth and normals, vertices in random order", shuffled[0], shuffled[1], depth))
        for what, vertices, nrm, dep in forms:
            baker.reset(V)
            baker.accumulate(vertices, V, cam, image, W, H, nrm, dep)
            one = baker.stats()
            t = timed(dev, lambda: baker.accumulate(vertices, V, cam, image, W, H, nrm, dep), ("mesh_bake_accumulate",))
            nbytes = (24 if nrm is not None else 12) * V + 72 * one["accumulated"]
            t.update(one_view=one, bytes=int(nbytes), bound_us=nbytes / STREAM_BYTES_PER_US, over_bound=t["sum_us"] / (nbytes / STREAM_BYTES_PER_US),
                     over_encode=t["sum_us"] / out["encode"]["sum_us"])
            out[f"accumulate, {what}"] = t
        out["resolve"] = timed(dev, lambda: baker.resolve(colours, V, mesh.get("colours"), mask), ("mesh_bake_resolve",))
        out["resolve"]["baked"] = baker.stats()["bakedVertices"]
    finally:
        for o in (rasterizer, baker, depth, colours, mask):
            o.destroy()
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshbake_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import _lib, ops, synth
    dev = ops.HipDevice(0)
    W, H = 1920, 1080
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.setdefault("note", "kernel times: the library's event-bracketed launches of one call, per kernel the median of five, in microseconds; host-clock times in ms, "
                              "each call followed by a wait; bound_us: the vertex and row bytes at 6.1 TB/s; over_bound and over_encode: the accumulate's time over "
                              "that bound and over the encode of the same mesh and view in the same run")
    v, f, col = sphere()
    centre = np.array([0.0, 0.0, 8.0])
    n = v.astype(np.float64) - centre
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    fine = upload(dev, v, f, col)
    fine_normals = dev.bufferFrom(n)
    order = np.random.default_rng(2).permutation(v.shape[0])
    shuffled = (dev.bufferFrom(np.ascontiguousarray(v[order])), dev.bufferFrom(np.ascontiguousarray(n[order])))
    cam = dev.bufferFrom(synth.camera_block(np.eye(4), W, H, H / 0.9))
    image = dev.bufferFrom(np.random.default_rng(1).integers(0, 256, (H, W, 4)).astype(np.uint8))
    coarse = ops.simplifyMesh(dev, fine, 2 * 8.0 / 512, origin=(-4.0, -4.0, 4.0), asBuffers=True)
    _, coarse_normals, _ = ops._smooth_and_normals(dev, coarse["vertices"], coarse["faces"], coarse["numVertices"], coarse["numFaces"], None, True)
    section = result.setdefault("builds", {}).setdefault(args.label, {})
    section["library"] = os.path.basename(_lib.LIB_PATH)
    section["sphere, 3.92 M faces"] = measure_mesh(dev, ops, f"sphere, 3.92 M faces ({args.label})", fine, fine_normals, cam, image, W, H, shuffled)
    section["simplify 2 voxels"] = measure_mesh(dev, ops, f"simplify 2 voxels ({args.label})", coarse, coarse_normals, cam, image, W, H)
    for m in (fine, coarse):
        ops.destroyBuffers({k: b for k, b in m.items() if isinstance(b, ops.HipBuffer)})
    for b in (fine_normals, coarse_normals, cam, image) + shuffled:
        b.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
