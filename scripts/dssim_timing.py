#!/usr/bin/env python3
"""Exact D-SSIM loss (trainingConfig dssim_mode="gaussian"): what it costs and what it trains to.

    python scripts/dssim_timing.py kernels [out_dir]        per-kernel times of loss_grad and dssim_grad at c2 (640x480) and c3 (1920x1080), from
                                                            rocprofv3 --kernel-trace --stats in a run of its own (this script under the profiler);
                                                            out_dir (default profiles/) gets dssim_kernel_stats_c2_c3.json and the two
                                                            dssim_<config>_kernel_stats.csv
    python scripts/dssim_timing.py step [steps] [blocks]    c3 single-view step time in both modes, the profiler off, the modes alternated block by
                                                            block in one process (default 40 steps, 4 blocks per mode)
    python scripts/dssim_timing.py quality [steps]          held-out PSNR and SSIM after the same number of steps in both modes, on one synthetic
                                                            scene (the setting of tests/test_gpu_eval.py::test_held_out_psnr_and_ssim_rise_over_training)

Each prints one JSON line at the end.  Needs an MI355X.
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from webdgs_amd import loaders, ops, synth  # noqa: E402
from webdgs_amd.trainer import Trainer  # noqa: E402

MODES = ("reference", "gaussian")


def _target_views(dev, cfg, n, width=None, height=None):
    """n views of the perturbed target scene, rendered by the same forward pass (the ground truth the synthetic cloud trains towards)."""
    w, h = width or cfg.width, height or cfg.height
    g, sh = synth.make_gaussians(cfg)
    tg, tsh = synth.make_target_scene(g, sh)
    cams = synth.circle_cameras(cfg, n)
    tpc = ops.createPointCloud(dev, tg, tsh, cfg.sh_deg)
    tcam = dev.createBuffer(272)
    tfw = ops.TiledForwardPass(dev, tpc, tcam, dict(viewportWidth=w, viewportHeight=h, renderMode="gaussian"))
    trs = ops.TiledRasterizer(dict(device=dev, forwardPass=tfw, format="rgba8unorm"))
    cameras, images = [], []
    for i in range(n):
        tcam.write(cams[i])
        tfw.encode(None)
        trs.encode(None, w, h)
        images.append(dict(texture=dev.bufferFrom(trs.getOutputTextureView().read(np.uint8)), width=w, height=h))
        cameras.append(dict(camera=cams[i], width=w, height=h))
    trs.destroy()
    tfw.destroy()
    return g, sh, tg, tsh, cameras, images


# ----------------------------------------------------------------------------- kernels
def _loss_calls(calls: int, name: str) -> None:
    """Runs under the profiler: computeLossOnly in both modes at one config on a rendered prediction and its target."""
    dev = ops.HipDevice(0)
    cfg = synth.CONFIGS[name]
    g, sh, _, _, cameras, images = _target_views(dev, cfg, 1)
    pc = ops.createPointCloud(dev, g, sh, cfg.sh_deg)
    cam = dev.bufferFrom(np.asarray(cameras[0]["camera"], np.float32))
    fw = ops.TiledForwardPass(dev, pc, cam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    rs = ops.TiledRasterizer(dict(device=dev, forwardPass=fw, format="rgba8unorm"))
    fw.encode(None)
    rs.encode(None, cfg.width, cfg.height)
    for mode in MODES:
        bwd = ops.TiledBackwardPass(dev, pc, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, trainingConfig=dict(dssim_mode=mode)))
        for _ in range(calls):
            bwd.computeLossOnly(None, rs.getOutputTextureView(), images[0]["texture"])
        dev.synchronize()
        bwd.destroy()
    rs.destroy()
    fw.destroy()
    print(f"{name}: {calls} calls per mode", flush=True)
    dev.destroy()


def kernels(out_dir: str, calls: int = 200) -> dict:
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    for name in ("c2", "c3"):
        d = tempfile.mkdtemp(prefix=f"dssim_rocprof_{name}_")   # the profiler's raw output; its kernel_stats.csv is kept in out_dir
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "_loss_calls", str(calls), name]
        subprocess.run(cmd, check=True, timeout=600)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert stats, f"no kernel_stats.csv under {d}"
        shutil.copyfile(stats[0], os.path.join(out_dir, f"dssim_{name}_kernel_stats.csv"))
        rows = {}
        with open(stats[0]) as f:
            for r in csv.DictReader(f):
                for k in ("loss_grad_kernel", "dssim_grad_kernel"):
                    if k in r["Name"]:
                        rows[k.replace("_kernel", "")] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                                              max_us=float(r["MaxNs"]) / 1e3)
        cfg = synth.CONFIGS[name]
        res[name] = dict(width=cfg.width, height=cfg.height, **rows)
        print(f"{name} {cfg.width}x{cfg.height}: " + ", ".join(f"{k} {v['avg_us']:.1f} us (min {v['min_us']:.1f}, {v['calls']} calls)" for k, v in rows.items()),
              flush=True)
        shutil.rmtree(d, ignore_errors=True)
    with open(os.path.join(out_dir, "dssim_kernel_stats_c2_c3.json"), "w") as f:
        json.dump(res, f, indent=1)
    return res


# ----------------------------------------------------------------------------- step
def step(steps: int, blocks: int) -> dict:
    dev = ops.HipDevice(0)
    cfg = synth.CONFIGS["c3"]
    g, sh, _, _, cameras, images = _target_views(dev, cfg, 8)
    t = Trainer(dev, seed=0)
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset(cameras, images)
    t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
    t.start()
    times = {m: [] for m in MODES}
    for m in MODES:   # warm-up: both modes' recordings and first launches
        t.setTrainingConfig(dict(dssim_mode=m))
        for _ in range(5):
            t.step()
        t.drain()
    for b in range(blocks):
        for m in (MODES if b % 2 == 0 else MODES[::-1]):
            t.setTrainingConfig(dict(dssim_mode=m))
            t.step()   # (re-records the step's command buffers)
            t.drain()
            t0 = time.perf_counter()
            for _ in range(steps):
                t.step()
            t.drain()
            times[m].append(1e3 * (time.perf_counter() - t0) / steps)
    t.destroy()
    dev.destroy()
    res = {m: dict(ms_per_step_median=float(np.median(v)), ms_per_step_blocks=[round(x, 4) for x in v]) for m, v in times.items()}
    res["gaussian_minus_reference_ms"] = res["gaussian"]["ms_per_step_median"] - res["reference"]["ms_per_step_median"]
    print(f"c3 step: reference {res['reference']['ms_per_step_median']:.3f} ms, gaussian {res['gaussian']['ms_per_step_median']:.3f} ms "
          f"({steps} steps x {blocks} blocks per mode, alternated)", flush=True)
    return dict(config="c3", width=cfg.width, height=cfg.height, gaussians=cfg.num_points, steps_per_block=steps, blocks=blocks, **res)


# ----------------------------------------------------------------------------- quality
def quality(steps: int) -> dict:
    dev = ops.HipDevice(0)
    c = synth.CONFIGS["c2"]
    cfg = synth.SceneConfig(c.config_id, 4000, 160, 128, 0, c.fy, 0.02, c.name + "-var")
    g, sh, tg, tsh, cameras, images = _target_views(dev, cfg, 24)
    trc, tri, tec, tei = loaders.holdoutSplit(cameras, images)
    # the model: the target's geometry with every Gaussian's colour scrambled; colours and opacities learn, the geometry stays
    h16 = tsh.copy().view(np.uint16).reshape(-1, 48)
    dc = h16[:, 0:3].view(np.float16).astype(np.float32) + np.random.default_rng(7).normal(0.0, 0.5, (len(h16), 3)).astype(np.float32)
    h16[:, 0:3] = synth.f32_to_f16_bits(dc)
    res = {}
    for m in MODES:
        t = Trainer(dev, seed=11, trainingConfig=dict(dssim_mode=m))
        t.setPointCloud(ops.createPointCloud(dev, tg, h16.view(np.uint32).reshape(-1, 24), cfg.sh_deg))
        t.setDataset(trc, tri)
        t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
        t.start()
        t.setOptimizerHyperparameters(dict(lr_pos=0.0, lr_rot=0.0, lr_scale=0.0))
        t.setEvaluationViews(tec, tei)
        r0 = t.evaluate()
        for _ in range(steps):
            t.step()
        r1 = t.evaluate()
        t.destroy()
        res[m] = dict(psnr_start=r0["mean_psnr"], ssim_start=r0["mean_ssim"], psnr=r1["mean_psnr"], ssim=r1["mean_ssim"])
        print(f"{m}: held-out PSNR {r0['mean_psnr']:.3f} -> {r1['mean_psnr']:.3f} dB, SSIM {r0['mean_ssim']:.5f} -> {r1['mean_ssim']:.5f} after {steps} steps",
              flush=True)
    dev.destroy()
    return dict(scene="c2 geometry, 4000 Gaussians, SH 0, 160x128, 21 train / 3 held-out views, colours scrambled", steps=steps, **res)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "step"
    if what == "_loss_calls":
        _loss_calls(int(sys.argv[2]), sys.argv[3])
        return
    if what == "kernels":
        out = kernels(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles"))
    elif what == "step":
        out = step(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    elif what == "quality":
        out = quality(int(sys.argv[2]) if len(sys.argv) > 2 else 400)
    else:
        raise SystemExit(__doc__)
    print(json.dumps({f"dssim_{what}": out}))


if __name__ == "__main__":
    main()
