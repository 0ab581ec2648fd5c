#!/usr/bin/env python3
"""Contribution timing: the contribution kernel beside rasterize in the same process and frames, at BASELINE scene sizes.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/contrib_timing.py [configs] [frames]
                                                                                      (default: c2,c3 200; needs an MI355X)

Every frame is forward encode + rasterize + encodeContribution on the synthetic cloud (identity camera) into one buffer, cleared every frame as a
caller would per view set, so the profiler's kernel statistics hold both kernels over the same frames.  Without a profiler the script prints the
library's own event-bracketed kernel times of a last, profiled pass.
`python scripts/contrib_timing.py --table <kernel_stats.csv> [...]` prints the two kernels' rows of profiler outputs as one table.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(paths):
    for path in paths:
        rows = {}
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for key in ("contribution_kernel", "rasterize_kernel<true"):
                    if key in r["Name"]:
                        rows[key] = r
        d, c = rows.get("contribution_kernel"), rows.get("rasterize_kernel<true")
        if not d or not c:
            print(f"{path}: kernels not found")
            continue
        da, ca = float(d["AverageNs"]) / 1e3, float(c["AverageNs"]) / 1e3
        print(f"{path}: rasterize {ca:.1f} us avg over {c['Calls']} calls (min {float(c['MinNs']) / 1e3:.1f}, max {float(c['MaxNs']) / 1e3:.1f}); "
              f"contribution {da:.1f} us avg over {d['Calls']} calls (min {float(d['MinNs']) / 1e3:.1f}, max {float(d['MaxNs']) / 1e3:.1f}); "
              f"ratio {da / ca:.3f}")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        return table(sys.argv[2:])
    from webdgs_amd import ops, synth
    configs = (sys.argv[1] if len(sys.argv) > 1 else "c2,c3").split(",")
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dev = ops.HipDevice(0)
    for name in configs:
        cfg = synth.CONFIGS[name]
        g, sh = synth.make_gaussians(cfg)
        pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
        cam = dev.bufferFrom(synth.identity_camera(cfg))
        fwd = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
        rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fwd, format="rgba8unorm"))
        stats = ops.createContributionBuffer(dev, cfg.num_points)

        def frame():
            fwd.encode(None)
            rast.encode(None, cfg.width, cfg.height)
            stats.clear()
            rast.encodeContribution(None, stats)

        frame()
        fwd.check()   # (a list that outran the pass would make the numbers meaningless: raises)
        for _ in range(frames):
            frame()
        dev.synchronize()
        dev.kernelTimes(reset=True)
        dev.setProfiling(True)
        for _ in range(20):
            frame()
        dev.synchronize()
        dev.setProfiling(False)
        kt = dev.kernelTimes(reset=True)
        r_n, r_ms = kt.get("rasterize", (0, 0.0))
        d_n, d_ms = kt.get("contribution", (0, 0.0))
        r_us, d_us = 1e3 * r_ms / max(1, r_n), 1e3 * d_ms / max(1, d_n)
        print(f"{name}: {cfg.num_points} Gaussians, {cfg.width}x{cfg.height}, E = {int(fwd.check()[0])}, {frames} frames; library event times over 20 "
              f"more: rasterize {r_us:.1f} us, contribution {d_us:.1f} us, ratio {d_us / max(r_us, 1e-9):.3f}", flush=True)
        got = ops.readContribution(stats, cfg.num_points)
        print(f"{name}: {int((got['pixels'] > 0).sum())} of {cfg.num_points} Gaussians composited, {int(got['pixels'].sum())} active pairs, weight {got['weight_sum'].sum():.1f}", flush=True)
        stats.destroy()
        rast.destroy()
        fwd.destroy()
        pc.gaussian_3d_buffer.destroy()
        pc.sh_buffer.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
