#!/usr/bin/env python3
"""The mesh rasterizer on the device: per-kernel times and host-clock times on a fine sphere, on its simplifications and on adversarial shapes.

    python scripts/meshraster_timing.py [--part all|grid] [--label NAME] [--out profiles/meshraster_timing.json]    (needs an MI355X)

Shapes (--part all):
  sphere:       a latitude-longitude sphere of 1400 x 1400 quads (3.92 M faces, 1.96 M vertices; radius 3 at distance 8, about 0.9 of the image's height) and
                ops.simplifyMesh of it at cells of 2, 4 and 8 "voxels" of 8 / 512, at 1920 x 1080 and 640 x 480, with the depth image alone and with all four;
  layers:       a hundred faces that each fill 1920 x 1080, given back to front (the early-out never fires: every fragment is a minimum) and front to back;
  one-pixel:    a million faces over one pixel centre, nearer and nearer: every atomic goes to one address;
  grid:         the viewport tiled by right triangles whose bounding boxes hold exactly n x n pixel centres, n from 4 to 64: with n at most
                WDGS_MESH_RASTER_LARGE_FACE_PIXELS the one-thread-per-face kernel draws them, above it the kernel of 8 x 8 blocks.  Run under builds of the
                library with other thresholds (WDGS_LIB_PATH; make VARIANT=_t8 EXTRA=-DWDGS_MESH_RASTER_LARGE_FACE_PIXELS=8u) with --part grid --label t8, the
                results are merged into the same file, with the simplified spheres at 1920 x 1080 under that build (sphere_by_threshold): where the two
                kernels cross is what the threshold is chosen by.
Per shape: per kernel the median of the library's event-bracketed times over five encodes, the host's clock around an encode and a wait (medians of five), the
statistics, and bytes_min -- 12 F of faces, 12 V of positions, 20 V of vertex records written and 60 F read back, 8 W H of z-buffer cleared and 8 W H read, and the
outputs -- to set against the 6.1 TB/s that consecutive 16-byte elements stream at on the same box.  fragments is the number of covered
(face, pixel) pairs, counted on the host for the crafted shapes: the upper bound on the atomics (the early-out skips those that cannot win).  The yardstick
`rasterize_c3` is the forward pass's compositing kernel on the c3 scene, same process.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("raster_vertices", "raster_faces", "raster_blocks", "raster_resolve", "scan_reduce", "scan_block_sums", "scan_downsweep")
BYTES = dict(depth=4, face=4, colour=4, normal=16)


def wall(dev, fn, runs=5):
    out = []
    for _ in range(runs):
        dev.synchronize()
        t0 = time.perf_counter()
        fn()
        dev.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=float(np.median(out)), ms_runs=out)


def kernel_times(dev, fn, names=KERNELS, runs=5):
    per, launches = {k: [] for k in names}, {}
    for _ in range(runs):
        dev.synchronize()
        dev.kernelTimes(reset=True)
        dev.setProfiling(True)
        fn()
        dev.synchronize()
        dev.setProfiling(False)
        kt = dev.kernelTimes(reset=True)
        for k in names:
            per[k].append(1e3 * kt.get(k, (0, 0.0))[1])
            launches[k] = kt.get(k, (0, 0.0))[0]
    med = {k: float(np.median(v)) for k, v in per.items() if launches[k]}
    return dict(kernels_us_median=med, sum_us=float(sum(med.values())))


def crafted_camera(W, H):
    c = np.zeros(68, np.float32)
    c[[0, 5, 10, 15]] = 1
    c[32] = c[37] = 1
    c[64], c[65] = W, H
    return c


def at(sx, sy, z, W, H):
    """View-space positions that the crafted camera puts at pixel coordinates (sx, sy) and depth z (arrays)."""
    sx, sy, z = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64), np.asarray(z, np.float64))
    return np.stack([(sx / W - 0.5) * 2.0 * z, -(sy / H - 0.5) * 2.0 * z, z], axis=-1)


def sphere(n_lat=1400, n_lon=1400, radius=3.0, centre=(0.0, 0.0, 8.0)):
    """A closed latitude-longitude sphere, two faces per quad (those at the poles degenerate), with colours."""
    th = np.linspace(0.0, np.pi, n_lat + 1)[:, None]
    ph = (np.arange(n_lon) * (2.0 * np.pi / n_lon))[None, :]
    v = np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], axis=-1).reshape(-1, 3) * radius + np.asarray(centre)
    i, j = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    a, b, c, d = i * n_lon + j, i * n_lon + (j + 1) % n_lon, (i + 1) * n_lon + j, (i + 1) * n_lon + (j + 1) % n_lon
    f = np.concatenate([np.stack([a, b, c], axis=-1).reshape(-1, 3), np.stack([b, d, c], axis=-1).reshape(-1, 3)])
    col = np.full((v.shape[0], 4), 255, np.uint8)
    col[:, :3] = (127.5 + 127.5 * np.sin(3.0 * v)).astype(np.uint8)
    return v.astype(np.float32), f.astype(np.uint32), col


def layers(n, W, H, front_to_back):
    z = 2.0 + 0.05 * np.arange(n)
    z = z if front_to_back else z[::-1]
    v = np.concatenate([at([-10.0, 2.0 * W + 10.0, -10.0], [-10.0, -10.0, 2.0 * H + 10.0], zk, W, H) for zk in z])
    f = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    return v.astype(np.float32), f, None, n * W * H


def one_pixel(n, W, H):
    z = (4.0 - 3.0 * np.arange(n) / n)[:, None]     # nearer and nearer: every fragment wins
    px, py = W // 2 + 0.5, H // 2 + 0.5
    v = at(np.array([px - 0.4, px + 0.4, px])[None, :], np.array([py - 0.3, py - 0.3, py + 0.4])[None, :], z, W, H).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), None, n


def grid(n, W, H):
    """Right triangles of legs n - 0.5 pixels from (k n + 0.25, l n + 0.25): each bounding box holds n x n pixel centres, the triangle n (n - 1) / 2 of them."""
    x0, y0 = np.meshgrid(np.arange(W // n) * n + 0.25, np.arange(H // n) * n + 0.25, indexing="ij")
    x0, y0 = x0.reshape(-1), y0.reshape(-1)
    z = 2.0 + 0.001 * np.arange(x0.size)
    v = np.stack([at(x0, y0, z, W, H), at(x0 + n - 0.5, y0, z, W, H), at(x0, y0 + n - 0.5, z, W, H)], axis=1).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * x0.size, dtype=np.uint32).reshape(-1, 3), None, None   # (no two overlap: the fragments are the covered pixels)


def measure(dev, ops, name, mesh, cam, W, H, outputs, fragments=None, runs=5):
    V, F = mesh["numVertices"], mesh["numFaces"]
    r = ops.MeshRasterizer(dev)
    outs = {k: dev.createBuffer(BYTES[k] * W * H) for k in outputs}
    try:
        fn = lambda: r.encode(mesh["vertices"], V, mesh["faces"], F, mesh.get("colours"), cam, W, H, **outs)   # noqa: E731
        fn()
        out = dict(vertices=V, faces=F, width=W, height=H, outputs=list(outputs), stats=r.stats(),
                   bytes_min=12 * F + 12 * V + 20 * V + 60 * F + 16 * W * H + sum(BYTES[k] for k in outputs) * W * H)
        if fragments is not None:
            out["fragments"] = int(fragments)
        fn()
        out.update(kernel_times(dev, fn, runs=runs), host_clock=wall(dev, fn, runs))
        out["GBps_of_bytes_min"] = out["bytes_min"] / out["sum_us"] / 1e3
    finally:
        r.destroy()
        for b in outs.values():
            b.destroy()
    print(name, json.dumps(out), flush=True)
    return out


def upload(dev, v, f, col=None):
    return dict(vertices=dev.bufferFrom(v), faces=dev.bufferFrom(f), colours=None if col is None else dev.bufferFrom(col), numVertices=v.shape[0], numFaces=f.shape[0])


def rasterize_c3(dev, ops):
    from webdgs_amd import synth
    cfg = synth.CONFIGS["c3"]
    g, sh = synth.make_gaussians(cfg)
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    cam = dev.bufferFrom(synth.identity_camera(cfg))
    fwd = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fwd, format="rgba8unorm"))

    def frame():
        fwd.encode(None)
        rast.encode(None, cfg.width, cfg.height)
    frame()
    out = dict(kernel_times(dev, frame, names=("rasterize",)), width=cfg.width, height=cfg.height, points=cfg.num_points)
    rast.destroy()
    fwd.destroy()
    print("rasterize_c3", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("all", "grid"))
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshraster_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import _lib, ops, synth
    dev = ops.HipDevice(0)
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.setdefault("note", "kernel times: the library's event-bracketed launches of one encode, per kernel the median of five, in microseconds; host-clock times in ms, "
                              "each encode followed by a wait; bytes_min over the sum of the kernel times in GB/s")
    W, H = 1920, 1080
    cam = dev.bufferFrom(crafted_camera(W, H))
    if args.part == "all":
        result["threshold"] = _lib.MESH_RASTER_LARGE_FACE_PIXELS
        result["rasterize_c3"] = rasterize_c3(dev, ops)
        v, f, col = sphere()
        fine = upload(dev, v, f, col)
        voxel = 8.0 / 512
        meshes = [("fine", fine)] + [(f"simplify {k} voxels", ops.simplifyMesh(dev, fine, k * voxel, origin=(-4.0, -4.0, 4.0), asBuffers=True)) for k in (2, 4, 8)]
        result["sphere"] = {}
        for w, h in ((1920, 1080), (640, 480)):
            view = np.eye(4)
            c = dev.bufferFrom(synth.camera_block(view, w, h, h / 0.9))
            for name, m in meshes:
                for outputs in (("depth",), ("depth", "face", "colour", "normal")):
                    key = f"{name}, {w}x{h}, {len(outputs)} output{'s' if len(outputs) > 1 else ''}"
                    result["sphere"][key] = measure(dev, ops, key, m, c, w, h, outputs)
            c.destroy()
        for _, m in meshes:
            ops.destroyBuffers({k: b for k, b in m.items() if isinstance(b, ops.HipBuffer)})
        result["adversarial"] = {}
        for name, shape in (("100 layers, back to front", layers(100, W, H, False)), ("100 layers, front to back", layers(100, W, H, True)),
                            ("1 M faces on one pixel", one_pixel(1000000, W, H))):
            v, f, _, fragments = shape
            m = upload(dev, v, f)
            result["adversarial"][name] = measure(dev, ops, name, m, cam, W, H, ("depth",), fragments, runs=3)
            ops.destroyBuffers({k: b for k, b in m.items() if isinstance(b, ops.HipBuffer)})
    else:   # the simplified spheres again, under this build's threshold
        v, f, col = sphere()
        fine = upload(dev, v, f, col)
        c = dev.bufferFrom(synth.camera_block(np.eye(4), W, H, H / 0.9))
        result.setdefault("sphere_by_threshold", {})[args.label] = {}
        for k in (2, 4, 8):
            m = ops.simplifyMesh(dev, fine, k * 8.0 / 512, origin=(-4.0, -4.0, 4.0), asBuffers=True)
            result["sphere_by_threshold"][args.label][f"simplify {k} voxels"] = measure(dev, ops, f"simplify {k} voxels ({args.label})", m, c, W, H, ("depth",))
            ops.destroyBuffers({k2: b for k2, b in m.items() if isinstance(b, ops.HipBuffer)})
        ops.destroyBuffers({k2: b for k2, b in fine.items() if isinstance(b, ops.HipBuffer)})
        c.destroy()
    result.setdefault("grid", {})[args.label] = {}
    for n in (4, 8, 12, 16, 17, 24, 32, 48, 64):
        v, f, _, fragments = grid(n, W, H)
        m = upload(dev, v, f)
        result["grid"][args.label][str(n)] = measure(dev, ops, f"grid of {n} x {n} ({args.label})", m, cam, W, H, ("depth",), fragments, runs=3)
        ops.destroyBuffers({k: b for k, b in m.items() if isinstance(b, ops.HipBuffer)})
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
