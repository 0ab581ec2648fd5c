#!/usr/bin/env python3
"""Texture baking on the device: per-kernel times of one view of a 2 M-face mesh.

    python scripts/meshtexture_timing.py [--label default] [--out profiles/meshtexture_timing.json]    (needs an MI355X)

Mesh: the latitude-longitude sphere of scripts/meshraster_timing.py at 1000 x 1000 quads (2.0 M faces, 1.0 M vertices), in cells of 8 texels (64 M texel rows,
1 GiB of state), under a 1920 x 1080 camera with a noise photograph.  Medians of five of the library's event-bracketed kernel times, in microseconds:
  encode                MeshRasterizer.encode with the depth image: the work that feeds one accumulate;
  vertex accumulate     MeshColourBaker.accumulate of the same mesh and view (depth and normals);
  typical               MeshTextureBaker.accumulate under the camera that looks at the sphere: the far half faces away, the silhouette is occluded;
  whole mesh            the same camera two-sided and without the depth image: every face in the image reaches its rows;
  none                  a camera that looks the other way: every face is behind the near plane and every wave leaves at the face-level test;
  typical, shuffled     the typical view over the same faces in random order: gathers without locality;
  resolve               MeshTextureBaker.resolve with vertex colours and the state image.
bound_us is the time the bytes that must move would take at the 6.1 TB/s that consecutive 16-byte elements stream at:
12 bytes of indices per face, 12 of position per vertex (each vertex read once), and 16 read and 16 written per texel that reaches its row; the photograph
and the depth image are not counted.  The 6.1 TB/s is section 5's figure (scripts/microbench/hbm_stream.hip), not a rate taken in
this run: every over_bound ratio rests on it.
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
CELL = 8


def timed(dev, fn, names):
    fn()
    return dict(kernel_times(dev, fn, names=names), host_clock_ms=wall(dev, fn)["ms_median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshtexture_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import _lib, ops, synth
    dev = ops.HipDevice(0)
    W, H = 1920, 1080
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.setdefault("note", "kernel times: the library's event-bracketed launches of one call, per kernel the median of five, in microseconds; host-clock times in ms, "
                              "each call followed by a wait; bound_us: the index, position and row bytes at 6.1 TB/s -- DESIGN.md section 5's streaming rate, not one measured in this run; over_bound and over_encode: the accumulate's time "
                              "over that bound and over the encode of the same mesh and view in the same run")
    v, f, col = sphere(1000, 1000)
    V, F = v.shape[0], f.shape[0]
    n = v.astype(np.float64) - np.array([0.0, 0.0, 8.0])
    normals = dev.bufferFrom((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    mesh = upload(dev, v, f, col)
    shuffled = dev.bufferFrom(np.ascontiguousarray(f[np.random.default_rng(2).permutation(F)]))
    cam = dev.bufferFrom(synth.camera_block(np.eye(4), W, H, H / 0.9))
    away = dev.bufferFrom(synth.camera_block(np.diag([-1.0, 1.0, -1.0, 1.0]), W, H, H / 0.9))
    image = dev.bufferFrom(np.random.default_rng(1).integers(0, 256, (H, W, 4)).astype(np.uint8))
    rasterizer, baker, vertex_baker = ops.MeshRasterizer(dev), ops.MeshTextureBaker(dev), ops.MeshColourBaker(dev)
    depth = dev.createBuffer(4 * W * H)
    L = baker.reset(F, CELL)
    texture, state = dev.createBuffer(4 * L["width"] * L["height"]), dev.createBuffer(L["width"] * L["height"])
    out = dict(library=os.path.basename(_lib.LIB_PATH), vertices=V, faces=F, width=W, height=H, cell=CELL, atlas=[L["width"], L["height"]])
    out["encode"] = timed(dev, lambda: rasterizer.encode(mesh["vertices"], V, mesh["faces"], F, None, cam, W, H, depth=depth), RASTER)
    vertex_baker.reset(V)
    out["vertex accumulate"] = timed(dev, lambda: vertex_baker.accumulate(mesh["vertices"], V, cam, image, W, H, normals, depth), ("mesh_bake_accumulate",))
    cases = (("typical", mesh["faces"], cam, depth, False), ("whole mesh", mesh["faces"], cam, None, True), ("none", mesh["faces"], away, depth, False),
             ("typical, shuffled", shuffled, cam, depth, False))
    for what, faces, camera, dep, two_sided in cases:
        baker.reset(F, CELL)
        call = lambda: baker.accumulate(mesh["vertices"], V, faces, F, camera, image, W, H, dep, twoSided=two_sided)
        call()
        one = baker.stats()
        t = timed(dev, call, ("mesh_texture_accumulate",))
        nbytes = 12 * F + 12 * V + 32 * one["accumulated"]
        t.update(one_view=one, bytes=int(nbytes), bound_us=nbytes / STREAM_BYTES_PER_US, over_bound=t["sum_us"] / (nbytes / STREAM_BYTES_PER_US),
                 over_encode=t["sum_us"] / out["encode"]["sum_us"], over_vertex_accumulate=t["sum_us"] / out["vertex accumulate"]["sum_us"])
        out[f"accumulate, {what}"] = t
        print(what, json.dumps(t), flush=True)
    baker.reset(F, CELL)
    baker.accumulate(mesh["vertices"], V, mesh["faces"], F, cam, image, W, H, depth)
    out["resolve"] = timed(dev, lambda: baker.resolve(mesh["faces"], F, V, texture, mesh["colours"], state), ("mesh_texture_resolve",))
    out["resolve"]["totals"] = baker.stats()
    print(json.dumps(out), flush=True)
    result.setdefault("builds", {})[args.label] = out
    for o in (rasterizer, baker, vertex_baker, depth, texture, state, normals, shuffled, cam, away, image):
        o.destroy()
    ops.destroyBuffers({k: b for k, b in mesh.items() if isinstance(b, ops.HipBuffer)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
