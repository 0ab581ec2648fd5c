#!/usr/bin/env python3
"""Mesh adjacency, Taubin smoothing and vertex normals on the device: per-kernel times and host-clock times on fused TSDF meshes and on adversarial shapes.

    python scripts/meshsmooth_timing.py [--sizes 256,512] [--views 8] [--out profiles/meshsmooth_timing.json]    (needs an MI355X)

The meshes are those of scripts/meshweld_timing.py: the c2 scene fused into a cube of 256^3 and of 512^3 voxels, welded on the device and left there.  For each:
  kernels:  per kernel the median of the library's event-bracketed times over five calls of count, emit, one iteration (two steps), ten iterations and normals;
  host:     count, one step, ten iterations and normals by the host's clock (medians of five), each followed by a wait.
step_bytes is what one smoothing step must move at least -- 12 V read, 12 V written, 8 (V + 1) of row starts, 4 V of boundary flags, 4 E of indices; the
gathers of 12 E bytes come on top where they miss the caches -- to set against the hbm_stream rate in profiles/.  The yardstick for count is the device weld's
one sort at the same size (profiles/meshweld_timing.json).  The adversarial shapes take the 512^3 mesh's V and F (or --adversarial-vertices /
--adversarial-faces): isolated vertices with a few faces at the end, at that V; and, at --long-row (200 000) because ONE lane walks a row and the time grows
with its length -- the time per element is the bound it is -- a fan whose hub has V - 1 = long-row neighbours, and every face the same triple (one edge key of
multiplicity long-row per direction; the normals of its three vertices each walk 2 long-row slots).  Last, the two-sphere volume of the tests, scored against points on the two
analytic spheres with and without smoothing, and with smoothing then simplification.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from meshweld_timing import fused_volumes  # noqa: E402

OWN = ("adjacency_half_edge_keys", "adjacency_fold", "adjacency_edges", "adjacency_rows", "adjacency_emit", "adjacency_copy", "adjacency_smooth_step",
       "adjacency_vertex_normals")
SORT = ("weld_key_bits", "weld_plan", "weld_histogram", "weld_scatter", "weld_heads")
SCAN = ("scan_reduce", "scan_block_sums", "scan_downsweep")
KERNELS = OWN + SORT + SCAN


def wall(dev, fn, runs=5):
    out = []
    for _ in range(runs):
        dev.synchronize()
        t0 = time.perf_counter()
        fn()
        dev.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=float(np.median(out)), ms_runs=out)


def kernel_times(dev, fn, runs=5):
    """Per kernel the median over ``runs`` calls of ``fn`` of the summed event times in microseconds, and the launches of one call."""
    per, launches = {k: [] for k in KERNELS}, {}
    for _ in range(runs):
        dev.synchronize()
        dev.kernelTimes(reset=True)
        dev.setProfiling(True)
        fn()
        dev.synchronize()
        dev.setProfiling(False)
        kt = dev.kernelTimes(reset=True)
        for k in KERNELS:
            per[k].append(1e3 * kt.get(k, (0, 0.0))[1])
            launches[k] = kt.get(k, (0, 0.0))[0]
    med = {k: float(np.median(v)) for k, v in per.items() if launches[k]}
    return dict(kernels_us_median=med, launches={k: n for k, n in launches.items() if n}, sum_us=float(sum(med.values())))


def measure(dev, ops, name, mesh, iterations=10, runs=5, pin=True):
    """mesh: dict(vertices, faces as HipBuffer, numVertices, numFaces); pin: smoothMesh's pinBoundary."""
    V, F = mesh["numVertices"], mesh["numFaces"]
    out = dict(vertices=V, faces=F, pin_boundary=pin)
    adj = ops.MeshAdjacency(dev)
    try:
        E = adj.count(mesh["faces"], F, V)
        bufs = [dev.createBuffer(n) for n in (4 * (V + 1), 4 * E, 4 * V, 12 * V, 12 * V)]
        count = lambda: adj.count(mesh["faces"], F, V)                                    # noqa: E731
        emit = lambda: adj.emit(bufs[0], bufs[1], bufs[2], E)                             # noqa: E731
        one = lambda: adj.smooth(mesh["vertices"], bufs[3], V, 1, pinBoundary=pin)                         # noqa: E731
        many = lambda: adj.smooth(mesh["vertices"], bufs[3], V, iterations, pinBoundary=pin)               # noqa: E731
        normals = lambda: adj.normals(mesh["vertices"], mesh["faces"], V, F, bufs[4])     # noqa: E731
        count()
        out.update(stats=adj.stats(), directed_edges=E)
        out["step_bytes"] = 12 * V + 12 * V + 8 * (V + 1) + 4 * V + 4 * E
        out["gather_bytes"] = 12 * E
        for key, fn in (("count", count), ("emit", emit), ("one_iteration", one), (f"{iterations}_iterations", many), ("normals", normals)):
            fn()
            out[key] = dict(kernel_times(dev, fn, runs), host_clock=wall(dev, fn, runs))
        step_us = out["one_iteration"]["kernels_us_median"]["adjacency_smooth_step"] / 2.0
        out["step_us"] = step_us
        out["step_GBps_of_step_bytes"] = out["step_bytes"] / step_us / 1e3
        out["step_GBps_with_gathers"] = (out["step_bytes"] + out["gather_bytes"]) / step_us / 1e3
        for b in bufs:
            b.destroy()
    finally:
        adj.destroy()
    print(name, json.dumps(out), flush=True)
    return out


def adversarial(V, F, long_row):
    """(name, faces u32[F', 3], V') of the three shapes."""
    i = np.arange(long_row - 1, dtype=np.int64)
    fan = np.stack([np.zeros_like(i), i + 1, i + 2], axis=1)                       # the hub 0 has long_row neighbours
    same = np.tile(np.array([[0, 1, 2]], np.int64), (long_row, 1))                  # one triple long_row times
    tail = np.stack([V - 3 + 0 * np.arange(4), V - 2 + 0 * np.arange(4), V - 1 + 0 * np.arange(4)], axis=1)   # V - 3 isolated vertices, a few faces at the end
    return (("fan", fan, long_row + 1), ("same-triple", same, V), ("isolated", tail, V))


def two_spheres(dev, ops):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meshclean_ref as M
    both, _, wt, rgb = M.two_sphere_fields()
    vol = ops.TSDFVolume(dev, M.TS_ORIGIN, M.TS_VOXEL, M.TS_DIMS, truncation=M.TS_TRUNC, colour=True)
    vol.getTSDFBuffer().write(np.ascontiguousarray(both, np.float32))
    vol.getWeightBuffer().write(np.ascontiguousarray(wt, np.float32))
    vol.getColourBuffer().write(np.ascontiguousarray(rgb, np.float32))
    rng = np.random.default_rng(31)
    ref = []
    for s in (M.TS_A, M.TS_B):
        d = rng.normal(size=(20000, 3))
        ref.append(s["centre"] + s["radius"] * d / np.linalg.norm(d, axis=1, keepdims=True))
    ref = np.concatenate(ref).astype(np.float32)
    out = {}
    cell = 2.0 * M.TS_VOXEL
    for name, options in (("raw", {}), ("smooth 3", dict(smooth=3)), ("smooth 10", dict(smooth=10)), ("2-voxel cells", dict(simplify=cell)),
                          ("smooth 3, then 2-voxel cells", dict(smooth=3, simplify=cell)), ("smooth 10, then 2-voxel cells", dict(smooth=10, simplify=cell))):
        mesh = vol.extractMesh(weld="device", **options)
        samples = ops.sampleMesh(dev, mesh, 1.0 / (0.5 * M.TS_VOXEL) ** 2, 0)
        m = ops.geometryMetrics(dev, samples["points"], ref, 8.0 * M.TS_VOXEL, M.TS_VOXEL)
        out[name] = dict(vertices=int(mesh["vertices"].shape[0]), faces=int(mesh["faces"].shape[0]),
                         **{k: float(m[k]) for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore")})
    plain = vol.extractMesh(weld="device")
    st = ops.meshAdjacency(dev, plain)["stats"]
    out["stats"] = dict(st, euler_characteristic=int(plain["vertices"].shape[0]) - st["edges"] + int(plain["faces"].shape[0]) - st["invalidFaces"])
    vol.destroy()
    print("two spheres", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--adversarial-vertices", type=int, default=0)
    ap.add_argument("--adversarial-faces", type=int, default=0)
    ap.add_argument("--long-row", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsmooth_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import ops
    dev = ops.HipDevice(0)
    result = dict(note="kernel times: the library's event-bracketed launches, per kernel the median of five calls, summed over the call's launches, in microseconds "
                       "(count: one sort -- eight histogram and scatter launches, those of skipped passes returning at once -- and ten scans: eight digit tables, the "
                       "head flags, the degrees; one iteration: two steps); host-clock times in ms, each call followed by a wait", tsdf={}, adversarial={})
    V = F = 0
    for size, tri in fused_volumes(dev, ops, [int(s) for s in args.sizes.split(",") if s], args.views):
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        V, F = welded["numVertices"], welded["numFaces"]
        result["tsdf"][str(size)] = measure(dev, ops, f"tsdf {size}^3", welded)
        ops.destroyBuffers(welded)
    V, F = args.adversarial_vertices or V, args.adversarial_faces or F
    if V >= 3 and F:
        positions = dev.bufferFrom(np.random.default_rng(29).uniform(-1.0, 1.0, (V, 3)).astype(np.float32))
        for name, faces, nv in adversarial(V, F, min(args.long_row, V - 1)):
            fb = dev.bufferFrom(np.ascontiguousarray(faces, np.uint32))
            result["adversarial"][name] = measure(dev, ops, f"{name} V={nv} F={faces.shape[0]}", dict(vertices=positions, faces=fb, numVertices=nv, numFaces=faces.shape[0]),
                                                  iterations=2, runs=2, pin=False)   # (every vertex of a fan is a boundary vertex)
            fb.destroy()
        positions.destroy()
    result["two_spheres"] = two_spheres(dev, ops)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
