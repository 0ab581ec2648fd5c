#!/usr/bin/env python3
"""bench.py -- training views/s (fwd + bwd + Adam) on BASELINE.json's headline configuration.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Invoked WITHOUT a launcher (`python bench.py --gpus N`, N > 1, no WORLD_SIZE in the environment) the process starts its N ranks itself:
before it imports torch or touches a GPU it spawns `python -m torch.distributed.run ... bench.py <same flags>` as a CHILD process, relays
that job's stdout (rank 0's JSON line), and exits with the child's return code (stderr tail on failure).

Workload: config c3 ("c3-perf": 1 M synthetic Gaussians, 1920x1080, SH degree 3), ground truth rendered by the
same HIP forward from the perturbed scene.  A training view = project -> scan -> emit -> sort -> ranges -> composite -> loss ->
backward raster -> geometry backward.

  N = 1   BASELINE config c3, the reference's own step: ONE view + fused Adam + re-pack per Trainer.step() (trainer.ts:568-660);
          8 circle cameras.  `value` = steps (= views) per second.
  N > 1   BASELINE config c4's shape: 64 circle cameras, `--views-per-rank` (default 8) views per rank per global step -- 64 global
          views at N = 8 -- summed locally in fp32, then ONE exchange per global step: reduce-scatter of the 60 B/Gaussian gradient
          block, Adam + re-pack on the owned 1/N slice, all-gather of the re-packed 32 B rows (webdgs_amd/parallel.py).  Weak
          scaling: the per-rank work (8 views) is fixed as N grows.  `value` = views per second of the whole job.  A rank deals its
          views to `--lanes` device lanes (default 3) so one view's bandwidth-bound stages run beside another's rasterization kernels.
          (`--views-per-rank 8` at N = 1 gives the single-GPU rate of the same 8-view step, the like-for-like base of the curve.)

The timed region is K Trainer.step() calls between a barrier + torch.cuda.synchronize() on both sides, max over ranks.  Submission
(`--pipeline-depth`, default 2): a step awaits the PREVIOUS step's completion ticket, so the host submits step k+1 while step k runs; every
one of the K steps has finished when the clock stops.  ONE JSON line on rank 0.

A plain run does only what the headline needs: set-up, W warm-up steps, ONE block of exactly K timed steps, the outputs of the last step
(`--dump-outputs DIR`), the JSON line.  `--full` adds everything else the record carries, after the timed region: the K-step block repeated
until `--min-seconds` have been timed (median block reported); the reference's await inside every step (trainer.ts:639-645) timed as
`ms_per_step_awaiting_every_step` (what `--pipeline-depth 1` makes the headline); an eager pass with hipEvents around every launch on the
launch stream (per-kernel averages, roofline of the dominant kernel); at N > 1 the exchange time and the single-GPU base of the same step; at
N = 1 the `batched_step` leg, a `sustained` leg (620 steps at the reference's densify defaults, crossing the first two densify events, carried
on to `full_run`) and the `cpu_baseline` (the oracle's train step built -O3 -march=native on this box's host cores).

`--dump-outputs DIR` writes, right after the timed region, what the last timed step left to the caller of Trainer.step(), as float32:
`gaussians.npy` (rows x 12: the trained fp16 Gaussian rows), `sh.npy` (rows x 48: their SH rows) and `image.npy` (pixels x 4: the rgba8
render of the step's view).  Above SAMPLE_ROWS Gaussians or SAMPLE_PIXELS pixels, a fixed seeded sample of them is written.  The reference's
densify schedule drives some Gaussians out of the fp16 range ("Non-finite Gaussians"): their NaN / +-infinity fields are written as
0 in `gaussians.npy` / `sh.npy` and named in `gaussians_nonfinite.npy` / `sh_nonfinite.npy` (same shape: 0 finite, 1 NaN, 2 +inf, 3 -inf), so
every array stays finite and comparable number for number.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def algorithmic_bytes(kernel: str, n: int, v: int, e: int, p: int, t: int, k_coef: int, passes: int, views: int = 1) -> float:
    """SURVEY.md section 8(d) per-stage algorithmic bytes for one training view (the view-batched kernels: for one step of `views` views)."""
    table = {
        "project_count": n * (24 + 6 * k_coef) + 28 * v + 4 * n,
        "scan": 8 * n,
        "emit": 16 * v + 8 * e,
        "sort": 4 * e + 16 * passes * e,
        "tile_ranges": 4 * e + 4 * (t + 1),
        "rasterize": 4 * e + 24 * v + 12 * p,
        "loss_grad": 24 * p,
        "backward_rasterize": 4 * e + 24 * v + 24 * p + 40 * v,
        "geometry_backward": 96 * n,
        "adam_repack": 4 * n + 416 * v + 100 * n,
        # K17 + K18 + K19 in one pass (single-view step): the packed gradient is written (32 N) but not read back
        "geometry_backward_adam": 96 * n + 4 * n + 416 * v + 100 * n - 32 * n,
        # the view-batched K1 / K17: Gaussian and SH row once per step, per view the splat, depth and count / the
        # accumulator row read and put back to zero, then the step's fp32 gradient row and visibility count written once
        "project_count_views": n * (24 + 6 * k_coef) + views * (28 * v + 4 * n),
        "geometry_backward_views": 24 * n + views * (96 * n + 4 * n) + 60 * n,
    }
    return float(table.get(kernel, 0))


def kernel_group(name: str) -> str:
    if name.startswith("sort_") or name.startswith("scan_"):
        return "sort" if name.startswith("sort_") else "scan"
    if name.startswith("tile_ranges"):
        return "tile_ranges"
    if name.startswith("adam_repack"):
        return "adam_repack"
    if name.startswith("emit"):  # emit, or emit fused with the sort's first pass (emit_scatter)
        return "emit"
    return name


def head_commit() -> str:
    try:
        import subprocess
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return ""


def make_dataset(dev, cfg, tg, tsh, cams):
    """Ground-truth images: HIP forward of the perturbed scene (oracle-free product path); resident rgba8 buffers."""
    from webdgs_amd import ops
    tpc = ops.createPointCloud(dev, tg, tsh, cfg.sh_deg)
    tcam = dev.createBuffer(272)
    tfw = ops.TiledForwardPass(dev, tpc, tcam, dict(viewportWidth=cfg.width, viewportHeight=cfg.height, renderMode="gaussian"))
    trs = ops.TiledRasterizer(dict(device=dev, forwardPass=tfw, format="rgba8unorm"))
    images, cameras = [], []
    for i in range(len(cams)):
        tcam.write(cams[i])
        tfw.encode(None)
        trs.encode(None, cfg.width, cfg.height)
        dev.synchronize()
        images.append(dict(texture=dev.bufferFrom(trs.getOutputTextureView().read(np.uint8)), width=cfg.width, height=cfg.height))
        cameras.append(dict(camera=cams[i], width=cfg.width, height=cfg.height))
    trs.destroy()
    tfw.destroy()
    return cameras, images


def probe_tile_lists(trainer, cfg, camera) -> tuple:
    """(tile entries E, length of the longest per-tile list) of the cloud as it is now under `camera`: one eager forward pass through the trainer's
    own passes (a preview render, as the reference's API allows between steps) and a host evaluation of its range table.  Not training time."""
    trainer.flushPointCloud()
    trainer.cameraBuffer.write(camera)
    trainer.forwardPass.encode(None)
    trainer.rasterizer.encode(None, cfg.width, cfg.height)
    e = int(trainer.forwardPass.check()[0])
    r = trainer.rasterizer.getTileOffsetsBuffer().read(np.uint32, cfg.total_tiles + 1).astype(np.int64)
    starts = r[:cfg.total_tiles]
    used = np.flatnonzero(starts != 0xFFFFFFFF)
    if used.size == 0:
        return e, 0
    ends = np.append(starts[used][1:], e)
    return e, int((ends - starts[used]).max())


def run_sustained(dev, cfg, g, sh, cameras, images, steps: int, pipeline_depth: int = 1, full_steps: int = 0) -> tuple:
    """BASELINE config c3 as written -- "full train loop with densify/prune schedule": a fresh Trainer at the reference's densify
    defaults (warm-up 500, every 100, 10 metric views at half resolution, <= 5000 new points per event).  Wall clock around every
    step(), densify events timed separately.  Two records come out of the ONE run: `sustained`, its first `steps` iterations (620: the
    first two densify events -- the figure earlier rounds reported), and `full_run`, the whole `full_steps` iterations (the reference's
    default training length, trainer.ts:73: maxIterations = 10 000) with the rate per window of 1 000 iterations, the point count,
    the tile entries and the longest tile list at each window's end -- the regime the first 620 iterations do not see (the schedule
    thins the cloud to a few per cent and collects thousands of non-finite Gaussians in tile 0)."""
    from webdgs_amd import ops
    from webdgs_amd.trainer import Trainer
    t = Trainer(dev, seed=99, pipeline_depth=pipeline_depth)
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset(cameras, images)
    t.setMaxIterations(10 ** 9)
    t.start()
    for _ in range(3):
        t.step()
    t.warmupCommandBuffers()
    dev.synchronize()
    start_it = t.getIteration()
    plain, events, sizes = [], [], [t.getPointCount()]
    t_all = time.perf_counter()
    sustained = None
    windows, w_t0, w_it0, excluded = [], t_all, start_it, 0.0
    last = max(steps, full_steps)
    while t.getIteration() < last:
        before = t.getLastDensifyPruneIteration()
        t0 = time.perf_counter()
        t.step()
        dt = time.perf_counter() - t0
        if t.getLastDensifyPruneIteration() != before:
            events.append(dt)
            sizes.append(t.getPointCount())
        else:
            plain.append(dt)
        it = t.getIteration()
        if it == steps and sustained is None:
            t.drain()
            dev.synchronize()
            total = time.perf_counter() - t_all - excluded
            n_steps = it - start_it
            # the steps right after a rebuild re-record their command buffers: count them with the event that caused them
            med = float(np.median(plain)) if plain else 0.0
            rerecord = float(sum(d - med for d in plain if d > 4.0 * med))
            sustained = dict(steps=n_steps, crosses_iterations=[start_it, it], iters_per_s_overall=round(n_steps / total, 2),
                             iters_per_s_steady=round(1.0 / med, 2) if med > 0 else None, ms_per_step_median=round(med * 1e3, 4), densify_events=len(events),
                             ms_per_densify_event=round((sum(events) + rerecord) / max(1, len(events)) * 1e3, 2) if events else None,
                             ms_per_densify_event_excluding_rerecording=round(float(np.mean(events)) * 1e3, 2) if events else None,
                             points=list(sizes), pipeline_depth=pipeline_depth,
                             schedule="reference defaults: warm-up 500, interval 100, 10 metric views at 1/2 resolution, maxNewPointsPerStep 5000")
        if full_steps and (it % 1000 == 0 or it == last) and it > w_it0:
            t.drain()
            dev.synchronize()
            now = time.perf_counter()
            tq = time.perf_counter()
            e_now, longest = probe_tile_lists(t, cfg, cameras[0]["camera"])
            windows.append(dict(to_iteration=it, iters_per_s=round((it - w_it0) / (now - w_t0), 1), points=t.getPointCount(), tile_entries_E=e_now,
                                longest_tile_list=longest))
            spent = time.perf_counter() - tq   # (the read-backs of the window record are not training time)
            excluded += spent
            w_t0, w_it0 = time.perf_counter(), it
    t.drain()
    dev.synchronize()
    full = None
    if full_steps:
        total = time.perf_counter() - t_all - excluded
        med_late = float(np.median(plain[-500:])) if plain else 0.0
        full = dict(iterations=t.getIteration() - start_it, iters_per_s_overall=round((t.getIteration() - start_it) / total, 2), seconds=round(total, 2),
                    densify_events=len(events), ms_per_step_median_last_500=round(med_late * 1e3, 4), windows=windows, final_points=t.getPointCount(),
                    pipeline_depth=pipeline_depth, note="BASELINE c3 as written, for the reference's default training length (trainer.ts:73: maxIterations = 10 000)")
    t.destroy()
    return sustained, full


def run_batched_step(dev, cfg, g, sh, tg, tsh, args, views_per_step: int = 8) -> dict:
    """The like-for-like base of the 1 -> 8 GPU curve, carried by the N = 1 record too: the SAME batched step a rank
    of an N > 1 job runs -- `views_per_step` views per step on the Trainer's default lanes, 64 circle cameras, recorded command buffers,
    the headline's pipeline depth, Adam on all N Gaussians, no exchange -- timed exactly like the headline (blocks of K steps from one
    restored training state, median block).  An N > 1 line divided by N x this rate is the scaling efficiency; dividing by the one-view
    `value` instead would flatter the curve (the one-view step is slower per view)."""
    from webdgs_amd import ops, parallel, synth
    from webdgs_amd.trainer import Trainer
    cams = synth.circle_cameras(cfg, 64)
    cameras, images = make_dataset(dev, cfg, tg, tsh, cams)
    t = Trainer(dev, seed=1234, world_size=1, rank=0, views_per_rank=views_per_step, overlap_views=args.lanes or None, pipeline_depth=args.pipeline_depth,
                exchange=parallel.Exchange())
    t.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    t.setDataset(cameras, images)
    t.setMaxIterations(10 ** 9)
    t.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
    t.start()
    steps = max(4, args.steps // 3)
    for _ in range(2):
        t.step()
    t.warmupCommandBuffers()
    el, _dev_ms, blocks, _ = timed_blocks(t, dev, steps, args.min_seconds, 1, barrier=lambda: None)
    out = dict(views_per_step=views_per_step, lanes=t._lanes, views_per_s=round(views_per_step * steps / el, 3), ms_per_step=round(el / steps * 1e3, 4), steps_per_block=steps,
               blocks=len(blocks), pipeline_depth=args.pipeline_depth, dataset_views=64,
               note="the per-rank step of BASELINE c4 on this one GPU: Adam on all N Gaussians, no exchange; the like-for-like base of an N > 1 line's value / N")
    t.destroy()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="c3", help="c3 (headline), c3-small, c2, c1, c5 -- only c3 is the BASELINE metric")
    ap.add_argument("--views", type=int, default=0, help="training views in the dataset (default: 8 at N = 1, 64 at N > 1)")
    ap.add_argument("--pipeline-depth", type=int, default=2, help="1: every step awaits its own completion (trainer.ts:639-645); 2: a step awaits the previous "
                    "one, so the host submits step k+1 while step k runs (the same K steps, all finished inside the timed region)")
    ap.add_argument("--lanes", type=int, default=0, help="device lanes a batched step deals its views to (0 = the Trainer's default; 1 = no overlap)")
    ap.add_argument("--views-per-rank", type=int, default=0, help="views per rank per global step (default: 1 at N = 1, 8 at N > 1)")
    ap.add_argument("--sustained-steps", type=int, default=620, help="N = 1: length of the densify-inclusive leg (0 = skip)")
    ap.add_argument("--full-run-steps", type=int, default=10_000, help="N = 1: the sustained leg goes on to this many iterations -- the reference's default training "
                    "length -- and reports the rate per window of 1 000 iterations (`full_run`; 0 = stop at --sustained-steps)")
    ap.add_argument("--full", action="store_true", help="also run every measurement besides the headline (repeated blocks, awaited leg, per-kernel pass and "
                    "roofline, exchange time, batched / sustained / full-run legs, CPU baseline); a plain run times one block of --steps steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    ap.add_argument("--min-seconds", type=float, default=None, help="the K-step block is repeated until this much time has been timed; the MEDIAN block is reported "
                    "(default: 1.0 with --full, else 0 = one block)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true", help="skip the eager per-kernel pass (roofline becomes null)")
    ap.add_argument("--no-batched-step", action="store_true", help="N = 1: skip the `batched_step` leg (the 8-views-per-step step of config c4 on this one GPU)")
    ap.add_argument("--no-single-gpu-base", action="store_true", help="N > 1: skip the like-for-like leg (the same batched step on rank 0 alone, no exchange)")
    ap.add_argument("--cpu-baseline-points", type=int, default=0, help="0 = full workload")
    args = ap.parse_args(argv)
    if args.min_seconds is None:
        args.min_seconds = 1.0 if args.full else 0.0
    return args


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return int(s.getsockname()[1])


def self_launch(n_ranks: int, argv: list) -> int:
    """`python bench.py --gpus N` from a bare shell: start the N ranks as a CHILD job (`python -m torch.distributed.run`, one rank per
    GPU) before this process has imported torch or touched a GPU, relay the job's stdout, return its exit code.  Nothing is exec'ed and
    no process that has initialised the GPU spawns another GPU program.  stderr of the job is kept in a temporary file and its tail is
    printed when the job fails (torchrun's own banner would otherwise bury the one JSON line of a good run)."""
    import signal
    import subprocess
    import tempfile
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, n_ranks))))
    env["WDGS_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__)] + list(argv)
    with tempfile.TemporaryFile(mode="w+") as err:
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=err, text=True, env=env, start_new_session=True)
        try:
            for line in proc.stdout:  # rank 0's JSON line goes to stdout; backend chatter (gloo prints its connection banner there) to stderr
                out = sys.stdout if line.lstrip().startswith("{") else sys.stderr
                out.write(line)
                out.flush()
            rc = proc.wait()
        except BaseException:  # Ctrl-C / a caller's timeout: take the whole job down (exactly the process group started above)
            try:
                os.killpg(proc.pid, signal.SIGTERM)
                proc.wait(timeout=20)
            except Exception:
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except Exception:
                    pass
            raise
        if rc != 0:
            err.seek(0)
            tail = err.read().splitlines()[-60:]
            print(f"[bench] the {n_ranks}-rank job exited with code {rc}; last lines of its stderr:", file=sys.stderr)
            for line in tail:
                print("    " + line, file=sys.stderr)
    return rc


def launcher_selftest() -> None:
    """WDGS_BENCH_SELFTEST=1: the body a rank runs in the launcher's CPU test (tests/test_bench_launcher.py) -- a gloo all-reduce of
    ones instead of the GPU workload, one JSON line on rank 0.  WDGS_BENCH_SELFTEST=fail makes rank 1 exit non-zero."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    if os.environ.get("WDGS_BENCH_SELFTEST") == "fail" and rank == world - 1:
        print("selftest: this rank fails on purpose", file=sys.stderr, flush=True)
        sys.exit(7)
    ones = torch.ones(1, dtype=torch.int32)
    if world > 1:
        dist.all_reduce(ones)
    if rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": world, "n_ranks_seen": int(ones.item()), "self_launched": os.environ.get("WDGS_BENCH_SELF_LAUNCHED") == "1",
                          "argv": sys.argv[1:]}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


class TrainingSnapshot:
    """Everything a block of steps changes -- point cloud, the six optimizer state arrays, the step counters, the view RNG -- kept in
    device copies so that every repeated block of the timed region starts from the SAME state and therefore times the SAME K steps
    (a training scene drifts: after 1300 steps c3's visible set has shrunk from 0.93 M to 0.22 M and a step costs 0.77 -> 1.17 ms).
    The restore runs OUTSIDE the timed bracket (device-to-device copies on the kernels' stream + a reload of the optimizer's compact
    SH-DC copy)."""

    def __init__(self, trainer):
        from webdgs_amd import parallel
        self.t = trainer
        dev = trainer.device
        pc = trainer.pointCloud
        trainer.flushPointCloud()                          # (deferred SH-DC halves -> the cloud's rows, which are what is copied)
        bufs = dict(trainer.optimizer.getStateBuffers())  # (flushes the compact SH-DC copy into paramSH / stateSH first)
        bufs.update(gaussians=pc.gaussian_3d_buffer, sh=pc.sh_buffer)
        self.views = {k: parallel._tensor_at(dev, b.ptr, b.size, __import__("torch").uint8) for k, b in bufs.items() if b.size > 0}
        self.copies = {k: v.clone() for k, v in self.views.items()}
        self.iteration, self.rng = trainer.iteration, trainer._rng.getstate()
        self.opt_iteration = trainer.optimizer.getIteration()

    def restore(self) -> None:
        t = self.t
        t.drain()
        t.flushPointCloud()
        for k, v in self.views.items():
            v.copy_(self.copies[k])
        t.optimizer.stateChanged()  # the compact SH-DC copy is reloaded from paramSH / stateSH
        if t.deferred_sh:
            t.optimizer.setDeferredSH(t.pointCloud, True)  # ... and the compact SH-DC halves from the restored rows
        t.optimizer.advanceIteration((self.opt_iteration - t.optimizer.getIteration()) & 0xFFFFFFFF)
        t.iteration = self.iteration
        t._rng.setstate(self.rng)


def timed_blocks(trainer, dev, steps: int, min_seconds: float, world: int, barrier=None):
    """The timed region: blocks of EXACTLY `steps` Trainer.step() calls, each bracketed by barrier + torch.cuda.synchronize() on both
    sides.  One block is the contract's measurement; it is repeated until `min_seconds` have been timed (every rank takes the same
    number of blocks: the count is fixed from the first block's max-over-ranks time) and the MEDIAN block is the one reported, so a
    16 ms region on a shared box is not at the mercy of one noisy neighbour.  Every block starts from the same training state
    (TrainingSnapshot, restored outside the bracket): the blocks time the same K steps.  Returns (median block seconds, max over
    ranks; device ms of that block; all block times; the exchange ms of that block when the trainer's `exchange_timing` is on, else 0)."""
    import torch
    from webdgs_amd import parallel
    if barrier is None:
        barrier = parallel.barrier
    snap = TrainingSnapshot(trainer) if min_seconds > 0 else None

    def one_block():
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record(dev.torch_stream)
        for _ in range(steps):
            trainer.step()
        trainer.drain()  # (pipeline depth 2: the last step's own await, with its deferred error check)
        ev1.record(dev.torch_stream)
        torch.cuda.synchronize()
        barrier()
        wall = time.perf_counter() - t0
        # (read after the bracket: the exchange intervals of THIS block, so the reported block's exchange time lies inside its own time)
        return wall, ev0.elapsed_time(ev1), trainer.exchangeMilliseconds() if trainer.exchange_timing else 0.0

    def max_over_ranks(values):
        if world <= 1 or not values:
            return list(values)
        import torch.distributed as dist
        t = torch.tensor(list(values), dtype=torch.float64, device=dev.torch_device)
        with parallel.collective_stream(dev.torch_device):  # (never on the stream the Trainer records on: parallel.collective_stream)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(x) for x in t.tolist()]

    first, first_dev, first_ex = one_block()
    first = max_over_ranks([first])[0]
    blocks, dev_ms, ex_ms = [first], [first_dev], [first_ex]
    n_more = 0 if min_seconds <= 0 else min(400, max(0, int(np.ceil(min_seconds / max(first, 1e-6))) - 1))
    for _ in range(n_more):
        snap.restore()
        e, d, x = one_block()
        blocks.append(e)
        dev_ms.append(d)
        ex_ms.append(x)
    blocks = [first] + max_over_ranks(blocks[1:])
    order = sorted(range(len(blocks)), key=lambda i: blocks[i])
    mid = order[(len(order) - 1) // 2]
    return blocks[mid], dev_ms[mid], blocks, ex_ms[mid]


def source_sha(kernel: str) -> str:
    """sha256 (16 hex) of the HIP source file a kernel lives in: ties an offline PMC profile to the kernel it describes."""
    import hashlib
    f = None
    for prefix, src in (("backward_rasterize", "backward_raster.hip"), ("rasterize", "raster.hip"), ("sort", "sort.hip"), ("segment_sort", "sort.hip"),
                        ("tile_ranges", "sort.hip"), ("project_count", "project.hip"), ("emit", "project.hip"), ("update_stats", "project.hip"),
                        ("geometry_backward", "backward.hip"), ("adam_repack", "optimizer.hip"), ("apply_rows", "optimizer.hip"), ("dc_", "optimizer.hip"),
                        ("unpack", "optimizer.hip"), ("loss_grad", "loss.hip"), ("scan", "scan.hip"), ("metric", "densify.hip"), ("densify", "densify.hip")):
        if kernel.startswith(prefix):
            f = src
            break
    if not f:
        return ""
    try:
        return hashlib.sha256(open(os.path.join(ROOT, "webdgs_amd", "csrc", f), "rb").read()).hexdigest()[:16]
    except OSError:
        return ""


def measured_issue_rate():
    """(wave-instructions per second, provenance) of the fastest plain fp32 VALU stream (v_fma / v_mul / v_add / v_sub_f32, one instruction kind per
    loop) in the newest committed record of scripts/microbench/valu_issue.hip at the rasterization kernels' occupancy (`profiles/*_valu_issue_w7.txt`);
    (None, reason) when there is none."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_valu_issue_w7.txt")), key=os.path.basename, reverse=True)
    for f in files:
        best = 0.0
        try:
            for ln in open(f):
                m = re.match(r"v_(?:fma|mul|add|sub)_f32\b.*?\s([\d.]+) G wave-instr/s", ln)
                if m:
                    best = max(best, float(m.group(1)))
        except OSError:
            continue
        if best > 0:
            return best * 1e9, f"profiles/{os.path.basename(f)}: fastest of the v_fma/v_mul/v_add/v_sub_f32 loops at 7 waves per SIMD (one box, one clock state)"
    return None, "no profiles/*_valu_issue_w7.txt record"


def build_roofline(dom: str, dur_ms: float, n: int, v: int, e: int, p_pix: int, tiles: int, k_coef: int, passes: int, config: str, pairs: int, raster_ms: float,
                   views: int = 1) -> dict:
    """The `roofline` object for the dominant kernel.  The two rasterization kernels (K14 / K16) are bound by fp32 VALU issue (SURVEY
    8(d)): for them `bound` = "valu_issue", achieved / peak are wave-instructions per second (a wave64 VALU instruction occupies its
    SIMD-32 for 2 cycles: 1024 SIMDs x 2.4 GHz / 2), the HBM fraction is kept as `hbm_frac` and SURVEY 8(d)'s flop fraction
    (F_fwd + F_bwd) / t / 157.3 TF as `flop_frac`.  VALU instruction counts and HBM traffic are PMC figures, which rocprofv3 collects in
    passes of their own (scripts/pmc.sh -> profiles/*_pmc.json): they are taken from the newest profile whose recorded hash of the
    kernel's source file equals the working tree's, and refused (null, with the reason) otherwise."""
    dur_s = dur_ms / 1e3
    abytes = algorithmic_bytes(dom, n, v, e, p_pix, tiles, k_coef, passes, views)
    hbm_gbps = abytes / dur_s / 1e9 if dur_s > 0 else 0.0
    roof = dict(bound="hbm", kernel=dom, achieved=round(hbm_gbps, 2), peak=8000.0, unit="GB/s", frac=round(hbm_gbps / 8000.0, 5), traffic=None,
                avg_ms_per_launch=round(dur_ms, 4), algorithmic_bytes=abytes, hbm_frac=round(hbm_gbps / 8000.0, 5))
    pmc_note = None
    prof = pk = None
    try:
        import glob
        refused = []
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")), key=os.path.basename, reverse=True):   # (names sort by round and pass: r03k > r02o > ...)
            cand = json.load(open(f))
            if cand.get("workload", "c3") != config or dom not in cand.get("kernels", {}) and dom not in ("sort", "scan"):
                continue
            want, have = source_sha(dom), (cand.get("source_sha") or {}).get(dom)
            if have != want:
                refused.append(os.path.basename(f))
                pmc_note = (f"no PMC profile of this version of {dom}'s source ({want}): refused " + ", ".join(refused[:3]) + (" ..." if len(refused) > 3 else "") +
                            " (recorded hash differs or is absent)")
                continue
            prof, pk, pmc_note = cand, cand["kernels"], f"offline PMC profile {os.path.basename(f)}" + (f" @ {cand['head']}" if cand.get("head") else "")
            break
    except Exception as exc:  # a missing or malformed profile must never break the bench line
        pmc_note = f"no PMC profile: {exc}"
    if pk is not None:
        names = {"sort": ("sort_hist", "sort_scan_rows", "sort_scatter", "sort_segments", "segment_sort", "emit_scatter"), "scan": ("scan_block_sums",)}.get(dom, (dom,))
        launches = {"sort_hist": 1, "sort_scan_rows": 1, "sort_scatter": 1}
        tr = sum(pk[nm].get("hbm_bytes", 0.0) * launches.get(nm, 1) for nm in names if nm in pk)
        if tr > 0:
            roof["traffic"] = round(tr)
            roof["traffic_over_algorithmic"] = round(tr / abytes, 3) if abytes else None
    roof["traffic_source"] = pmc_note
    if dom in ("rasterize", "backward_rasterize"):
        f_fwd, f_bwd = 256.0 * e * 23.0, 256.0 * e * 12.0 + pairs * 60.0   # SURVEY 8(d) "Algorithmic flops (raster)"
        flops = f_fwd if dom == "rasterize" else f_bwd
        roof["flop_frac"] = round(flops / dur_s / 157.3e12, 4) if dur_s > 0 else None
        roof["flop_frac_note"] = ("SURVEY 8(d)'s count charges every (pixel, entry) pair of the reference's loops; the kernels skip most of them (block culling, "
                                  "saturation), so this says how much work is avoided -- it can exceed 1 -- not how busy the pipes are: that is `frac`")
        if raster_ms > 0:
            roof["flop_frac_fwd_plus_bwd"] = round((f_fwd + f_bwd) / (raster_ms / 1e3) / 157.3e12, 4)
        peak_issue = 1024 * 2.4e9 / 2.0  # wave-instructions per second the chip can issue
        # What a stream of plain fp32 VALU instructions really sustains on this chip (the clock it holds under a full vector load is below
        # 2.4 GHz): read from the committed microbenchmark record, never a constant in this file -- null when the record is absent
        attainable, attainable_src = measured_issue_rate()
        insts = pk[dom].get("SQ_INSTS_VALU") if pk is not None and dom in pk else None
        roof.update(bound="valu_issue", unit="G wave-instr/s", peak=round(peak_issue / 1e9, 1), attainable_measured=round(attainable / 1e9, 1) if attainable else None,
                    attainable_source=attainable_src)
        if insts:
            roof.update(achieved=round(insts / dur_s / 1e9, 1), frac=round(insts / dur_s / peak_issue, 4),
                        frac_of_attainable=round(insts / dur_s / attainable, 4) if attainable else None, valu_insts_per_launch=round(insts))
        else:
            roof.update(achieved=None, frac=None, note="VALU instruction count needs a PMC profile of this kernel version (scripts/pmc.sh); hbm_frac and flop_frac are live")
    return roof


SAMPLE_ROWS, SAMPLE_PIXELS = 1 << 15, 1 << 21  # dumped Gaussians / pixels at most: 49 MB of float32 (c3's 1080p image fits whole)


def _sample(n: int, cap: int) -> np.ndarray:
    """All of range(n), or a fixed seeded sorted sample of `cap` of them: the same indices from run to run and build to build."""
    if n <= cap:
        return np.arange(n)
    return np.sort(np.random.default_rng(0).choice(n, cap, replace=False))


def _finite_split(a: np.ndarray) -> tuple:
    """(a with its non-finite entries set to 0, a code of the same shape: 0 finite, 1 NaN, 2 +inf, 3 -inf), both float32."""
    code = np.select([np.isnan(a), np.isposinf(a), np.isneginf(a)], [1, 2, 3], 0).astype(np.float32)
    return np.where(code == 0, a, 0).astype(np.float32), code


def dump_outputs(trainer, cfg, out_dir: str) -> None:
    """What the last timed step left to the caller of Trainer.step(): the trained point cloud and the step's render (module docstring)."""
    os.makedirs(out_dir, exist_ok=True)
    n = trainer.getPointCount()
    pc = trainer.pointCloud
    rows = _sample(n, SAMPLE_ROWS)
    g = pc.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6)[:n][rows]
    sh = pc.sh_buffer.read(np.uint32).reshape(-1, 24)[:n][rows]  # (the read brings deferred SH-DC rows up to date first)
    img = trainer.rasterizer.getOutputTextureView().read(np.uint8, cfg.width * cfg.height * 4).reshape(-1, 4)
    img = img[_sample(img.shape[0], SAMPLE_PIXELS)]
    for name, words in (("gaussians", g), ("sh", sh)):
        values, code = _finite_split(np.ascontiguousarray(words).view(np.float16).astype(np.float32))
        np.save(os.path.join(out_dir, f"{name}.npy"), values)
        np.save(os.path.join(out_dir, f"{name}_nonfinite.npy"), code)
    np.save(os.path.join(out_dir, "image.npy"), img.astype(np.float32))


def main() -> None:
    args = parse_args()
    if os.environ.get("WDGS_BENCH_SELFTEST") and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    if os.environ.get("WDGS_BENCH_SELFTEST"):
        launcher_selftest()
        return
    # `python bench.py --gpus N` with no launcher around it: become the launcher (before torch is imported or a GPU is touched)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))

    # WDGS_BENCH_WATCHDOG=<seconds>: if the run is still going after that long, every thread's Python stack goes to stderr and the
    # process exits -- a hung collective then names itself instead of running into the caller's timeout
    if os.environ.get("WDGS_BENCH_WATCHDOG"):
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["WDGS_BENCH_WATCHDOG"]), exit=True)

    import torch
    from webdgs_amd import ops, parallel, synth
    from webdgs_amd.trainer import Trainer

    rank, world, local_rank = parallel.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"[bench] WORLD_SIZE={world} but --gpus {args.gpus}: launch with torch.distributed.run --nproc-per-node {args.gpus} (or with no launcher at all)")
    # WDGS_FORCE_DEVICE (with WDGS_DIST_BACKEND=gloo): rehearse N > 1 on a single-GPU box; never set by the driver
    dev = ops.HipDevice(int(os.environ.get("WDGS_FORCE_DEVICE", local_rank)))
    vpr = args.views_per_rank or (1 if world == 1 else 8)
    n_dataset = args.views or (8 if world == 1 and vpr == 1 else 64)

    # ranks that really answer: an all-reduce of ones over the job's backend (RCCL on a multi-GPU node)
    n_ranks_seen = 1
    if world > 1:
        import torch.distributed as dist
        ones = torch.ones(1, dtype=torch.int32, device=dev.torch_device)
        with parallel.collective_stream(dev.torch_device):
            dist.all_reduce(ones)
        n_ranks_seen = int(ones.item())

    cfg = synth.CONFIGS[args.config]
    g, sh = synth.make_gaussians(cfg)
    tg, tsh = synth.make_target_scene(g, sh)
    cams = synth.circle_cameras(cfg, n_dataset)
    cameras, images = make_dataset(dev, cfg, tg, tsh, cams)

    trainer = Trainer(dev, seed=1234, world_size=world, rank=rank, views_per_rank=vpr, overlap_views=args.lanes or None, pipeline_depth=args.pipeline_depth)
    lanes = trainer._lanes
    trainer.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
    trainer.setDataset(cameras, images)
    trainer.setMaxIterations(10 ** 9)
    if vpr > 1 or world > 1:  # the headline leg of a batched run measures the step itself; densify is the N = 1 `sustained` leg
        trainer.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
    trainer.start()

    for _ in range(args.warmup):
        trainer.step()
    trainer.warmupCommandBuffers()  # every view's command buffer recorded before the clock starts (set-up, like pipeline creation)
    stats = trainer.forwardPass.check()  # raises on tile-entry overflow

    # ---- timed region: recorded command buffers (HIP graphs), no per-kernel events.  Device time of the same region from two
    # events on the kernels' own stream (it is torch's current stream: ops.HipDevice).
    trainer.exchange_timing = world > 1 and args.full
    elapsed, device_ms, blocks, exchange_ms = timed_blocks(trainer, dev, args.steps, args.min_seconds, world)
    if args.dump_outputs and rank == 0:  # (before any leg below takes steps of its own)
        dump_outputs(trainer, cfg, args.dump_outputs)
    #  the exchange events are switched off HERE, before the awaited leg below takes its own steps
    trainer.exchange_timing = False
    # the same K steps with the reference's own await inside every step (depth 1), for comparison; not the headline
    awaited_ms = None
    if args.full and trainer.pipeline_depth > 1:
        trainer.pipeline_depth = 1
        torch.cuda.synchronize()
        parallel.barrier()
        t_a = time.perf_counter()
        for _ in range(args.steps):
            trainer.step()
        torch.cuda.synchronize()
        parallel.barrier()
        awaited_ms = (time.perf_counter() - t_a) / args.steps * 1e3
        trainer.pipeline_depth = args.pipeline_depth
    if world > 1 and args.full:
        import torch.distributed as dist
        tt = torch.tensor([exchange_ms], dtype=torch.float64, device=dev.torch_device)
        with parallel.collective_stream(dev.torch_device):
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        exchange_ms = float(tt[0].item())

    # ---- per-kernel durations: the same K steps again, launched eagerly with a hipEvent pair around every kernel on the
    # launch stream (events cannot bracket single kernels inside a replayed graph).  Kernels, grids and data are identical.
    ktimes, eager_elapsed = {}, 0.0
    if args.full and not args.no_profile:
        trainer.use_command_buffers = False
        trainer._invalidate_command_buffers()
        trainer.step()
        dev.setProfiling(True)
        dev.kernelTimes(reset=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            trainer.step()
        torch.cuda.synchronize()
        eager_elapsed = time.perf_counter() - t1
        dev.setProfiling(False)
        ktimes = dev.kernelTimes()
        if not ktimes:
            raise RuntimeError("bench: the per-kernel leg recorded no kernel (roofline would be empty)")

    stats = trainer.forwardPass.check()
    e_entries, v_visible = int(stats[0]), int(stats[1])
    n, p_pix, tiles = cfg.num_points, cfg.width * cfg.height, cfg.total_tiles
    k_coef = (cfg.sh_deg + 1) ** 2
    key_bits = 16 + max(1, tiles).bit_length()
    passes = (key_bits + 7) // 8
    pairs = int(trainer.rasterizer.getNContribTextureView().read(np.uint32).astype(np.uint64).sum()) if args.full else None
    views_per_step = world * vpr

    # ---- roofline for the dominant kernel (group sort_* / scan_* launches into their stage); durations are PER VIEW
    groups: dict = {}
    for name, (launches, ms) in ktimes.items():
        gname = kernel_group(name)
        gl, gms = groups.get(gname, (0, 0.0))
        groups[gname] = (gl + launches, gms + ms)
    per_view_kernels = ("project_count", "scan", "emit", "sort", "tile_ranges", "rasterize", "loss_grad", "backward_rasterize", "geometry_backward", "geometry_backward_adam",
                        "store_gradients", "accumulate_gradients", "guard_accumulate", "acc_clear")
    per_step = {k: v[1] / max(1, args.steps) / (vpr if k in per_view_kernels else 1) for k, v in groups.items()}
    # (the dominant kernel by time per STEP: a per-view kernel runs once per view of the step)
    dom = max(per_step, key=lambda k: per_step[k] * (vpr if k in per_view_kernels else 1)) if per_step else None
    roofline = None
    if dom:
        roofline = build_roofline(dom, per_step[dom], n, v_visible, e_entries, p_pix, tiles, k_coef, passes, args.config, pairs,
                                  per_step.get("rasterize", 0.0) + per_step.get("backward_rasterize", 0.0), views=vpr)

    # every stage against the HBM roof (algorithmic bytes / live duration): the streaming stages are the ones it binds
    hbm_by_stage = {}
    for k, ms in per_step.items():
        ab = algorithmic_bytes(k, n, v_visible, e_entries, p_pix, tiles, k_coef, passes, vpr)
        if ab > 0 and ms > 0:
            hbm_by_stage[k] = dict(GBps=round(ab / (ms / 1e3) / 1e9, 1), frac=round(ab / (ms / 1e3) / 8.0e12, 4))

    ms_per_step = elapsed / args.steps * 1e3
    value = views_per_step * args.steps / elapsed

    # ---- N > 1: the like-for-like base of the scaling curve -- the SAME batched step (views per rank, lanes, recorded command
    # buffers, pipeline depth) on rank 0's GPU alone, without the exchange (the other ranks wait at the barrier).  The N = 1 bench line
    # is the reference's one-view step, which is a different (slower per view) step: dividing by it would flatter the curve.
    same_step = None
    if world > 1 and args.full and not args.no_single_gpu_base:
        trainer.use_command_buffers = True
        parallel.barrier()
        if rank == 0:
            solo = Trainer(dev, seed=1234, world_size=1, rank=0, views_per_rank=vpr, overlap_views=args.lanes or None, pipeline_depth=args.pipeline_depth,
                           exchange=parallel.Exchange())
            solo.setPointCloud(ops.createPointCloud(dev, g, sh, cfg.sh_deg))
            solo.setDataset(cameras, images)
            solo.setMaxIterations(10 ** 9)
            solo.setDensifyPruneConfig(dict(schedule=dict(enabled=False)))
            solo.start()
            for _ in range(args.warmup):
                solo.step()
            solo.warmupCommandBuffers()
            s_el, s_dev, s_blocks, _ = timed_blocks(solo, dev, args.steps, args.min_seconds, 1, barrier=lambda: None)
            same_step = dict(views_per_s=round(vpr * args.steps / s_el, 3), ms_per_step=round(s_el / args.steps * 1e3, 4), views_per_step=vpr, lanes=solo._lanes,
                             blocks=len(s_blocks), note="rank 0's GPU alone: same views per rank, lanes, command buffers and pipeline depth; Adam on all N Gaussians, no exchange")
            solo.destroy()
        parallel.barrier()

    sustained = cpu_baseline = batched = full_run = None
    if rank == 0 and world == 1 and args.full:
        trainer.destroy()
        if vpr == 1 and not args.no_batched_step and args.config in ("c3", "c3-small", "c2"):
            batched = run_batched_step(dev, cfg, g, sh, tg, tsh, args)
        if args.sustained_steps > 0 and args.config in ("c3", "c3-small", "c2"):
            sustained, full_run = run_sustained(dev, cfg, g, sh, cameras, images, args.sustained_steps, args.pipeline_depth,
                                                full_steps=args.full_run_steps)
        if not args.no_cpu_baseline:
            cpu_baseline = run_cpu_baseline(cfg, g, sh, cams[0], args.cpu_baseline_points)

    if rank == 0:
        exch = None
        if world > 1 and args.full:
            sl = parallel.slice_points(n, world)
            exch = dict(transport=trainer.exchange.name, ms_per_step=round(exchange_ms / args.steps, 4), frac_of_step=round(exchange_ms / args.steps / ms_per_step, 4),
                        bytes_sent_per_rank_per_step=int((world - 1) * sl * (60 + 32)),
                        note="device time between the events that bracket the two collectives of a step in the reported block (waiting for the slowest rank included)")
        out = {
            "metric": "training iters/sec (fwd+bwd+Adam), 1M Gaussians @1080p SH3" if args.config == "c3" else f"training iters/sec (fwd+bwd+Adam), {cfg.name}",
            "value": round(value, 3), "unit": "iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "device_ms_per_step": round(device_ms / args.steps, 4),
            "timed_blocks": dict(blocks=len(blocks), steps_per_block=args.steps, seconds_timed=round(sum(blocks), 4), reported="median block",
                                 ms_per_step_min=round(min(blocks) / args.steps * 1e3, 4), ms_per_step_max=round(max(blocks) / args.steps * 1e3, 4)),
            "ms_per_step_awaiting_every_step": round(awaited_ms, 4) if awaited_ms is not None else None,
            "eager_profiled_ms_per_step": round(eager_elapsed / args.steps * 1e3, 4) if ktimes else None,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "head": head_commit(),
            "n_ranks_seen": n_ranks_seen, "self_launched": os.environ.get("WDGS_BENCH_SELF_LAUNCHED") == "1", "full": args.full,
            "single_gpu_same_step": same_step,
            "scaling_efficiency": round(value / (world * same_step["views_per_s"]), 4) if same_step else None,
            # BASELINE c3 as written ("full train loop with densify/prune schedule"): the densify-inclusive rate of the `sustained` leg
            "c3_as_written_iters_per_s": sustained["iters_per_s_overall"] if sustained else None,
            # ... and the same run carried on to the reference's default training length (10 000 iterations): rate per 1 000-iteration window
            "c3_full_run_iters_per_s": full_run["iters_per_s_overall"] if full_run else None,
            "full_run": full_run,
            "config": {"workload": f"{cfg.name}: {n} Gaussians, {cfg.width}x{cfg.height}, SH deg {cfg.sh_deg}, fwd+bwd per view, {n_dataset} circle views"
                                   + (" (BASELINE c3: the reference's one-view step)" if views_per_step == 1 else f" (BASELINE c4 shape: {vpr} views per rank per global step)"),
                       "views_per_rank": vpr, "global_batch_views": views_per_step, "lanes": lanes,
                       "parallelism": (f"dp{world}: views sharded; per global step one reduce-scatter (60 B/Gaussian) -> Adam on the owned 1/{world} slice -> "
                                       f"all-gather (32 B/Gaussian) over RCCL") if world > 1 else "single GPU",
                       "tile_entries_E": e_entries, "visible_V": v_visible, "contributing_pairs_C_upper": pairs,
                       "pipeline_depth": args.pipeline_depth,
                       "submission": "recorded command buffers (HIP graphs), one per view, re-submitted; " +
                                     ("every step awaits its own completion, as the reference does" if args.pipeline_depth <= 1 else
                                      "a step awaits the PREVIOUS step's completion ticket (the host submits step k+1 while step k runs); all K steps "
                                      "finish inside the timed region; `ms_per_step_awaiting_every_step` is the reference's own await-per-step"),
                       "densify_schedule": "reference defaults (warm-up 500): not reached in the timed region; see `sustained` / `c3_as_written_iters_per_s`" if views_per_step == 1 else "disabled in this leg",
                       "iter_definition": "value counts training VIEWS (fwd+bwd) per second; a step = views_per_rank x n_gpus views + 1 exchange + 1 Adam"},
            # durations by the per-kernel events of the eager leg: kernels that run once per VIEW of a step, and kernels that run once per STEP
            # (the view-batched K1 / K17 and the optimizer pass of a batched step) -- never mixed in one table
            "kernel_ms_per_view": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1]) if k in per_view_kernels},
            "kernel_ms_per_step": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1]) if k not in per_view_kernels},
            "batched_step": batched,
            "roofline": roofline, "hbm_roofline_by_stage": hbm_by_stage, "exchange": exch, "sustained": sustained, "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)
    # orderly shutdown: every rank has finished its collectives; ops and command buffers, then the device, then the process group
    parallel.barrier()
    trainer.destroy()
    if getattr(trainer, "exchange", None) is not None:
        trainer.exchange.destroy()
    dev.destroy()
    parallel.shutdown()


def run_cpu_baseline(cfg, g, sh, cam, points: int) -> dict:
    """Times the oracle (the reference's path restated on the CPU, OpenMP over Gaussians/tiles/rows) on this box's host cores."""
    from oracle import oracle as orc
    from webdgs_amd import synth
    native = orc.use_native_build()  # -O3 -march=native, built here, on the box that times it
    cores = os.cpu_count() or 1
    os.environ.setdefault("OMP_NUM_THREADS", str(cores))
    if points and points < cfg.num_points:
        g, sh = g[:points].copy(), sh[:points].copy()
    else:
        g, sh = g.copy(), sh.copy()
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    tg, tsh = synth.make_target_scene(g, sh)
    target = orc.forward(tg, tsh, cam, st, ti)["rgba8"]
    state = orc.unpack(g, sh)
    t0 = time.perf_counter()
    iters = 0
    while True:
        orc.train_step(g, sh, state, cam, st, ti, target)
        iters += 1
        if time.perf_counter() - t0 > 10.0 or iters >= 5:
            break
    dt = time.perf_counter() - t0
    frac = g.shape[0] / cfg.num_points
    return dict(value=round(iters / dt, 4), unit="iters/s", cores=cores, kind="port",
                build="g++ -O3 -march=native -fopenmp" if native else "g++ -O3 -fopenmp (portable build: the native build failed)",
                sample=f"{iters} full training iteration(s) of {cfg.name} with {g.shape[0]} Gaussians ({frac:.0%} of the workload) on {cores} host threads (oracle = CPU restatement of the reference WGSL; the reference itself cannot run without a browser)",
                ms_per_step=round(dt / iters * 1e3, 1))


if __name__ == "__main__":
    main()
