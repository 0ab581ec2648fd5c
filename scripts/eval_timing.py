#!/usr/bin/env python3
"""Held-out evaluation timing: the SSIM kernel's average time (the library's own kernel times) and Trainer.evaluate throughput in views/s, at
BASELINE scene sizes (default c3: 1 M Gaussians at 1920x1080, and c5: 5 M at 3840x2160).  The model is the untrained synthetic cloud, the
ground truth the perturbed target scene rendered by the same forward pass; training state does not change what evaluate costs.

    python scripts/eval_timing.py [configs] [views] [repeats] [out.json]     (default: c3,c5 16 10; needs an MI355X)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from webdgs_amd import ops, synth  # noqa: E402
from webdgs_amd.trainer import Trainer  # noqa: E402


def measure(dev, name: str, views: int, repeats: int) -> dict:
    cfg = synth.CONFIGS[name]
    g, sh = synth.make_gaussians(cfg)
    tg, tsh = synth.make_target_scene(g, sh)
    cams = synth.circle_cameras(cfg, views)
    tpc = ops.createPointCloud(dev, tg, tsh, cfg.sh_deg)
    tcam = dev.createBuffer(272)
    tfw = ops.TiledForwardPass(dev, tpc, tcam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    trs = ops.TiledRasterizer(dict(device=dev, forwardPass=tfw, format="rgba8unorm"))
    cameras, images = [], []
    for i in range(views):
        tcam.write(cams[i])
        tfw.encode(None)
        trs.encode(None, cfg.width, cfg.height)
        images.append(dict(texture=dev.bufferFrom(trs.getOutputTextureView().read(np.uint8)), width=cfg.width, height=cfg.height))
        cameras.append(dict(camera=cams[i], width=cfg.width, height=cfg.height))
    trs.destroy()
    tfw.destroy()
    tpc.gaussian_3d_buffer.destroy()
    tpc.sh_buffer.destroy()

    t = Trainer(dev, seed=0)
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset(cameras[:1], images[:1])
    t.setEvaluationViews(cameras, images)
    first = t.evaluate()   # builds the evaluation passes (and grows their lists if a view needs it)
    t.evaluate()
    # kernel times: one profiled pass over the views
    dev.kernelTimes(reset=True)
    dev.setProfiling(True)
    t.evaluate()
    dev.setProfiling(False)
    kt = dev.kernelTimes(reset=True)
    # throughput, unprofiled
    t0 = time.perf_counter()
    for _ in range(repeats):
        r = t.evaluate()
    dt = time.perf_counter() - t0
    assert r["sse"] == first["sse"] and r["ssim"] == first["ssim"], "evaluate is not reproducible"
    ssim_n, ssim_ms = kt.get("image_ssim", (0, 0.0))
    fin_n, fin_ms = kt.get("image_ssim_finish", (0, 0.0))
    sse_n, sse_ms = kt.get("image_sse", (0, 0.0))
    per_view_ms = sum(ms for _, ms in kt.values()) / views
    out = dict(config=name, gaussians=cfg.num_points, width=cfg.width, height=cfg.height, views=views, repeats=repeats,
               ssim_kernel_us=1e3 * ssim_ms / max(1, ssim_n), ssim_finish_us=1e3 * fin_ms / max(1, fin_n), sse_kernel_us=1e3 * sse_ms / max(1, sse_n),
               kernel_ms_per_view=per_view_ms, views_per_s=views * repeats / dt, evaluate_ms=1e3 * dt / repeats,
               mean_psnr=r["mean_psnr"], mean_ssim=r["mean_ssim"],
               kernels_us={k: round(1e3 * ms / max(1, n), 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])})
    t.destroy()
    return out


def main():
    configs = (sys.argv[1] if len(sys.argv) > 1 else "c3,c5").split(",")
    views = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    path = sys.argv[4] if len(sys.argv) > 4 else None
    dev = ops.HipDevice(0)
    results = []
    for name in configs:
        m = measure(dev, name, views, repeats)
        results.append(m)
        print(f"{name}: {m['gaussians']} Gaussians, {m['width']}x{m['height']}: image_ssim {m['ssim_kernel_us']:.1f} us (+ finish {m['ssim_finish_us']:.1f} us), "
              f"image_sse {m['sse_kernel_us']:.1f} us, kernels {m['kernel_ms_per_view'] * 1e3:.0f} us per view, evaluate {m['views_per_s']:.0f} views/s "
              f"(held-out PSNR {m['mean_psnr']:.2f} dB, SSIM {m['mean_ssim']:.4f})", flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
    print(json.dumps(dict(eval_timing=[{k: v for k, v in m.items() if k != "kernels_us"} for m in results])))
    dev.destroy()


if __name__ == "__main__":
    main()
