#!/usr/bin/env python3
"""Simplification by vertex clustering on the device: per-kernel times and host-clock times on fused TSDF meshes and on the reduction's adversarial shapes.

    python scripts/meshsimplify_timing.py [--sizes 256,512] [--views 8] [--cells 2,4,8] [--out profiles/meshsimplify_timing.json]    (needs an MI355X)

The meshes are those of scripts/meshweld_timing.py: the c2 scene fused into a cube of 256^3 and of 512^3 voxels, welded on the device and left there.  Each
is simplified at cell sizes of 2, 4 and 8 voxels from the volume's origin:
  kernels:  per kernel the median of the library's event-bracketed times over five count + emit calls on the device-resident mesh;
  host:     the same count + emit into buffers made beforehand, and ops.simplifyMesh with its read-back, by the host's clock (medians of five).
The adversarial shapes take the 512^3 mesh's V and F (or --adversarial-vertices / --adversarial-faces): every vertex in one cell, every vertex in a cell
of its own, cell keys that differ only in their top byte.  stage_bytes is what each stage must move, to set against the hbm_stream rate in profiles/.
Last, the two-sphere volume of the tests: the simplified and the unsimplified mesh scored against points on the two analytic spheres.
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

OWN = ("simplify_cell_keys", "simplify_accumulate", "simplify_finalize", "simplify_face_keys", "simplify_fold", "simplify_face_keys2", "simplify_mark",
       "simplify_emit_vertices", "simplify_emit_faces")
SORT = ("weld_key_bits", "weld_plan", "weld_histogram", "weld_scatter", "weld_heads", "weld_emit")
SCAN = ("scan_reduce", "scan_block_sums", "scan_downsweep")
KERNELS = OWN + SORT + SCAN


def stage_bytes(V, F, colours):
    """The bytes each of the simplifier's own stages must read and write (the sorts' are meshweld_timing's 32 bytes per slot and pass)."""
    c = 4 if colours else 0
    return dict(simplify_cell_keys=(12 + 8) * V, simplify_accumulate=(12 + 4 + c) * V + 64 * V, simplify_face_keys=(12 + 3 * 8 + 3 * 4 + 8 + 4 + 4) * F,
                simplify_face_keys2=(4 + 4 + 8) * F, simplify_mark=(4 + 4 + 4 + 4) * F + 4 * V, simplify_emit_vertices=(4 + 4 + 8 + 4 + 4) * V,
                simplify_emit_faces=(4 + 4) * F)


def wall(fn, runs=5):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=float(np.median(out)), ms_runs=out)


def measure(dev, ops, name, mesh, origin, cell):
    """mesh: dict(vertices, faces, colours | None as HipBuffer, numVertices, numFaces)."""
    V, F, cols = mesh["numVertices"], mesh["numFaces"], mesh.get("colours")
    out = dict(vertices=V, faces=F, cell_size=float(cell))
    simp = ops.MeshSimplifier(dev)
    try:
        nv, nf = simp.count(mesh["vertices"], V, mesh["faces"], F, cols, origin, cell)
        outs = [dev.createBuffer(n) for n in (12 * nv, 12 * nf, 4 * nv, 8 * nv, 4 * nf, 4 * V)]

        def run():
            simp.count(mesh["vertices"], V, mesh["faces"], F, cols, origin, cell)
            simp.emit(mesh["vertices"], V, mesh["faces"], F, cols, outs[0], outs[1], outs[2] if cols is not None else None, outs[3], outs[4], outs[5], nv, nf)

        run()
        dev.synchronize()
        per, launches = {k: [] for k in KERNELS}, {}
        for _ in range(5):
            dev.kernelTimes(reset=True)
            dev.setProfiling(True)
            run()
            dev.synchronize()
            dev.setProfiling(False)
            kt = dev.kernelTimes(reset=True)
            for k in KERNELS:
                per[k].append(1e3 * kt.get(k, (0, 0.0))[1])
                launches[k] = kt.get(k, (0, 0.0))[0]
        med = {k: float(np.median(v)) for k, v in per.items()}
        group = lambda names: float(sum(med[k] for k in names))   # noqa: E731
        out.update(stats=simp.stats(), kernels_us_median=med, launches=launches, own_us=group(OWN), sorts_us=group(SORT), scans_us=group(SCAN),
                   kernels_sum_us=group(KERNELS), stage_bytes=stage_bytes(V, F, cols is not None))
        out["stage_GBps"] = {k: b / med[k] / 1e3 for k, b in out["stage_bytes"].items() if med[k] > 0}

        def count_emit():
            run()
            dev.synchronize()

        out["count_emit_host_clock"] = wall(count_emit)
        for b in outs:
            b.destroy()
    finally:
        simp.destroy()
    out["simplify_mesh_with_readback"] = wall(lambda: ops.simplifyMesh(dev, mesh, cell, origin))
    print(name, json.dumps(out), flush=True)
    return out


def adversarial(dev, V, F):
    """(name, vertices f32[V,3], cell) of the three shapes; faces are shared: (i, i + 1, i + 1024) mod V."""
    rng = np.random.default_rng(23)
    one = (rng.uniform(0.0, 1.0, (V, 3)) + 5.0).astype(np.float32)
    i = np.arange(V, dtype=np.int64)
    own = (np.stack([i % 1024, (i // 1024) % 1024, i // (1024 * 1024)], axis=1) + 0.5).astype(np.float32)
    top = np.zeros((V, 3), np.float32) + np.float32(0.5)
    top[:, 2] = (rng.integers(0, 128, V) * 16384 + 0.5).astype(np.float32)   # cz = k 2^14: bits 56..62 of the key
    return (("one-cell", one, 1.0), ("own-cell", own, 1.0), ("top-byte-only", top, 1.0))


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
    for name, simplify in (("unsimplified", None), ("2-voxel cells", 2.0 * M.TS_VOXEL), ("4-voxel cells", 4.0 * M.TS_VOXEL)):
        mesh = vol.extractMesh(weld="device", simplify=simplify)
        samples = ops.sampleMesh(dev, mesh, 1.0 / (0.5 * M.TS_VOXEL) ** 2, 0)
        m = ops.geometryMetrics(dev, samples["points"], ref, 8.0 * M.TS_VOXEL, M.TS_VOXEL)
        out[name] = dict(vertices=int(mesh["vertices"].shape[0]), faces=int(mesh["faces"].shape[0]),
                         **{k: float(m[k]) for k in ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore")})
    vol.destroy()
    print("two spheres", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--adversarial-vertices", type=int, default=0)
    ap.add_argument("--adversarial-faces", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsimplify_timing.json"))
    args = ap.parse_args()
    from webdgs_amd import ops
    dev = ops.HipDevice(0)
    result = dict(note="kernel times: the library's event-bracketed launches of one count + emit, per kernel the median of five calls (three sorts: 24 histogram and "
                       "scatter launches, those of skipped passes returning at once; 29 scans: 24 digit tables, three head-flag scans, the cluster and face flags); "
                       "host-clock times in ms", tsdf={}, adversarial={})
    origin = (-4.0, -4.0, 2.0)
    V = F = 0
    for size, tri in fused_volumes(dev, ops, [int(s) for s in args.sizes.split(",") if s], args.views):
        welded = ops.weldTrianglesDevice(dev, tri, asBuffers=True)
        V, F = welded["numVertices"], welded["numFaces"]
        for c in [float(x) for x in args.cells.split(",") if x]:
            result["tsdf"][f"{size}/{c:g}"] = measure(dev, ops, f"tsdf {size}^3, cells of {c:g} voxels", welded, origin, c * 8.0 / size)
        ops.destroyBuffers(welded)
    V, F = args.adversarial_vertices or V, args.adversarial_faces or F
    if V and F:
        i = np.arange(F, dtype=np.int64)
        faces = dev.bufferFrom(np.stack([i % V, (i + 1) % V, (i + 1024) % V], axis=1).astype(np.uint32))
        for name, vertices, cell in adversarial(dev, V, F):
            mesh = dict(vertices=dev.bufferFrom(vertices), faces=faces, colours=None, numVertices=V, numFaces=F)
            result["adversarial"][name] = measure(dev, ops, f"{name} V={V} F={F}", mesh, (0.0, 0.0, 0.0), cell)
            mesh["vertices"].destroy()
        faces.destroy()
    result["two_spheres"] = two_spheres(dev, ops)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    dev.destroy()


if __name__ == "__main__":
    main()
