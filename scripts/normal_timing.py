#!/usr/bin/env python3
"""Normal-map timing: the four normal kernels beside rasterize in the same process and frames, at BASELINE scene sizes.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/normal_timing.py [configs] [frames]
                                                                                      (default: c2,c3 200; needs an MI355X)

Every frame is forward encode + rasterize + encodeNormal (gaussian_normals, normal_composite) + encodeDepth(median) + depthToNormals + normalAgreement
on the synthetic cloud (identity camera), so the profiler's kernel statistics hold all of them over the same frames.  Without a profiler the script
prints the library's own event-bracketed kernel times of a last, profiled pass.
`python scripts/normal_timing.py --table <kernel_stats.csv> [...]` prints the kernels' rows of profiler outputs as one table.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("rasterize_kernel<true", "normal_composite_kernel", "depth_composite_kernel", "gaussian_normals_kernel", "depth_to_normals_kernel", "normal_agreement_kernel")


def table(paths):
    for path in paths:
        rows = {}
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for key in KERNELS:
                    if key in r["Name"]:
                        rows[key] = r
        if KERNELS[0] not in rows or KERNELS[1] not in rows:
            print(f"{path}: kernels not found")
            continue
        base = float(rows[KERNELS[0]]["AverageNs"])
        print(f"{path}:")
        for key in KERNELS:
            r = rows.get(key)
            if r:
                avg = float(r["AverageNs"])
                print(f"  {key.split('<')[0]:26s} {avg / 1e3:8.1f} us avg over {r['Calls']} calls (min {float(r['MinNs']) / 1e3:.1f}, max {float(r['MaxNs']) / 1e3:.1f}); "
                      f"{avg / base:.3f} x rasterize")


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
        block = synth.identity_camera(cfg)
        cam = dev.bufferFrom(block)
        fwd = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
        rast = ops.TiledRasterizer(dict(device=dev, forwardPass=fwd, format="rgba8unorm"))
        dn = dev.createBuffer(16 * cfg.width * cfg.height, "depth normals")
        sums = dev.createBuffer(24, "agreement")

        def frame():
            fwd.encode(None)
            rast.encode(None, cfg.width, cfg.height)
            rast.encodeNormal(None)
            rast.encodeDepth(None, ("median",))
            ops.depthToNormals(dev, rast.getDepthTextureView("median"), cfg.width, cfg.height, block, dn)
            ops.encodeNormalAgreement(dev, rast.getNormalTextureView(), dn, cfg.width, cfg.height, sums)

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
        us = {k: 1e3 * kt.get(k, (0, 0.0))[1] / max(1, kt.get(k, (0, 0.0))[0]) for k in
              ("rasterize", "normal_composite", "depth_composite", "gaussian_normals", "depth_to_normals", "normal_agreement")}
        e, a, cnt = (int(x) for x in sums.read("uint64", count=3))
        print(f"{name}: {cfg.num_points} Gaussians, {cfg.width}x{cfg.height}, E = {int(fwd.check()[0])}, {frames} frames; library event times over 20 more: "
              + ", ".join(f"{k} {v:.1f} us" for k, v in us.items()) + f"; normal_composite / rasterize {us['normal_composite'] / max(us['rasterize'], 1e-9):.3f}; "
              f"1 - cos = {e / max(a, 1):.6f} over {cnt} pixels", flush=True)
        for b in (dn, sums):
            b.destroy()
        rast.destroy()
        fwd.destroy()
        pc.gaussian_3d_buffer.destroy()
        pc.sh_buffer.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
