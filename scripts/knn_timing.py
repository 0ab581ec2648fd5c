#!/usr/bin/env python3
"""k-nearest query and neighbour-based scale initialisation timing at a million points.

    python scripts/knn_timing.py [points] [--out DIR]           (default: 1000000, profiles/; needs an MI355X)

Writes DIR/knn_timing.json and prints it.  Four measurements:

  list_cost    kNearest with k = 1 against nearest on the same index (uniform points in the unit cube) and the same queries, alternating, five calls
               each: the walk is the same and the pair counts are equal, so the difference is the cost of the list.  nearest is the yardstick.
  self_query   the indexed points as their own queries with the self-exclusion, k = 3, 8 and 16, at a cutoff of twice the extent: the early exit
               decides how far each query looks.  Pairs examined are counted in a separate untimed call.
  init_scales  initScalesFromNeighbours end to end on a cloud of as many points (positions unpacked, index built, self-query, scales written, two
               read-backs), by the host clock around the synchronising call, after one warm-up call.
  outliers     the shape a uniform grid handles worst: the same dense core plus eight points 50 extents away, at the default cutoff (twice the widest
               extent), and with maxDistance given.  One call each: the first takes long.

Kernel times are the library's own event-bracketed ones (HipDevice.kernelTimes); end-to-end times are host clocks around calls that end in a read-back.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def profiled(dev, fn):
    dev.synchronize()
    dev.kernelTimes(reset=True)
    dev.setProfiling(True)
    fn()
    dev.synchronize()
    dev.setProfiling(False)
    return {k: (int(c), 1e3 * float(ms)) for k, (c, ms) in dev.kernelTimes(reset=True).items()}


def records_from(positions):
    """u32[N, 6] records of a 'normal' cloud as the loaders make them: fp16 position, opacity 1, identity rotation, log sigma -5."""
    g = np.zeros((positions.shape[0], 12), np.float16)
    g[:, 0:3] = positions
    g[:, 3], g[:, 4] = 1.0, 1.0
    g[:, 8:11] = -5.0
    return np.ascontiguousarray(g).view(np.uint32).reshape(-1, 6)


def main():
    from webdgs_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("points", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    ap.add_argument("--skip-outliers", action="store_true")
    args = ap.parse_args()
    n = args.points
    dev = ops.HipDevice(0)
    rng = np.random.default_rng(1)
    pts = rng.random((n, 3)).astype(np.float32)
    qs = rng.random((n, 3)).astype(np.float32)
    result = dict(points=n)
    pbuf, qbuf = dev.bufferFrom(pts), dev.bufferFrom(qs)
    d2, idx, pairs = dev.createBuffer(4 * n * 16), dev.createBuffer(4 * n * 16), dev.createBuffer(8)

    def count_pairs(fn):
        pairs.clear()
        fn(pairs)
        dev.synchronize()
        return int(pairs.read(np.uint64, count=1)[0])

    # ---- list_cost: k = 1 against nearest
    cutoff = 2.0 * n ** (-1.0 / 3.0)
    index = ops.PointIndex(dev, pbuf, count=n)
    index.nearestInto(None, qbuf, n, cutoff, d2, idx)          # completes the build; warm
    index.kNearestInto(None, qbuf, n, 1, cutoff, d2, idx)
    near_us, k1_us = [], []
    for _ in range(5):
        near_us.append(profiled(dev, lambda: index.nearestInto(None, qbuf, n, cutoff, d2, idx))["nearest"][1])
        k1_us.append(profiled(dev, lambda: index.kNearestInto(None, qbuf, n, 1, cutoff, d2, idx))["k_nearest"][1])
    p_near = count_pairs(lambda p: index.nearestInto(None, qbuf, n, cutoff, d2, idx, p))
    p_k1 = count_pairs(lambda p: index.kNearestInto(None, qbuf, n, 1, cutoff, d2, idx, pairs=p))
    info = index.info()
    result["list_cost"] = dict(cutoff=cutoff, cell=info["cellSize"], dims=info["dims"], nearest_us=near_us, k1_us=k1_us, nearest_pairs=p_near, k1_pairs=p_k1,
                               nearest_us_median=float(np.median(near_us)), k1_us_median=float(np.median(k1_us)))
    print(json.dumps(result["list_cost"]), flush=True)

    # ---- self_query with the flag
    result["self_query"] = {}
    for k in (3, 8, 16):
        index.kNearestInto(None, pbuf, n, k, 2.0, d2, idx, True)      # warm
        us = [profiled(dev, lambda: index.kNearestInto(None, pbuf, n, k, 2.0, d2, idx, True))["k_nearest"][1] for _ in range(5)]
        examined = count_pairs(lambda p: index.kNearestInto(None, pbuf, n, k, 2.0, d2, idx, True, p))
        result["self_query"][str(k)] = dict(cutoff=2.0, k_nearest_us=us, k_nearest_us_median=float(np.median(us)), pairs=examined, pairs_per_query=examined / n)
        print(k, json.dumps(result["self_query"][str(k)]), flush=True)
    index.destroy()

    # ---- init_scales end to end
    core = (rng.random((n, 3)) * 8.0 - 4.0)
    g = records_from(core)
    sh = np.zeros((n, 24), np.uint32)
    pc = ops.createPointCloud(dev, g, sh, 0)
    ops.initScalesFromNeighbours(dev, pc)                             # warm
    times, kt = [], None
    for _ in range(3):
        pc.gaussian_3d_buffer.write(g)
        dev.synchronize()
        t0 = time.perf_counter()
        out = ops.initScalesFromNeighbours(dev, pc)
        times.append(1e3 * (time.perf_counter() - t0))
    pc.gaussian_3d_buffer.write(g)
    kt = profiled(dev, lambda: ops.initScalesFromNeighbours(dev, pc))
    result["init_scales"] = dict(k=3, ms=times, ms_median=float(np.median(times)), kernels_us={k: v[1] for k, v in kt.items()},
                                 found_3=int((out["found"] == 3).sum()), mean_sigma=float(np.sqrt(out["meanD2"][np.isfinite(out["meanD2"])]).mean()))
    print(json.dumps(result["init_scales"]), flush=True)

    # ---- outliers: a dense core and eight points 50 extents away
    if not args.skip_outliers:
        far = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * 50.0 * 8.0
        g2 = records_from(np.concatenate([core, far]))
        m = g2.shape[0]
        pc2 = ops.createPointCloud(dev, g2, np.zeros((m, 24), np.uint32), 0)
        result["outliers"] = {}
        for name, max_distance in (("max_distance_0.5", 0.5), ("default_cutoff", None)):
            pc2.gaussian_3d_buffer.write(g2)
            dev.synchronize()
            t0 = time.perf_counter()
            kt = profiled(dev, lambda: ops.initScalesFromNeighbours(dev, pc2, maxDistance=max_distance))
            ms = 1e3 * (time.perf_counter() - t0)
            result["outliers"][name] = dict(ms=ms, k_nearest_us=kt["k_nearest"][1], kernels_us={k: v[1] for k, v in kt.items()})
            print(name, json.dumps(result["outliers"][name]), flush=True)

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "knn_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    dev.destroy()


if __name__ == "__main__":
    main()
