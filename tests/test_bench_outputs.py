"""CPU: ``bench.py --dump-outputs DIR`` writes the last timed step's outputs as float32 .npy files, whole when small and as the same seeded
sample from run to run when large, with every value finite (non-finite fields are named in a code array of their own), within 64 MB at the
largest config (c5: 5 M Gaussians, 3840x2160).  The device reads are stood in for by
host arrays; the GPU run of the same path is tests/test_gpu_dp.py::test_plain_bench_line_times_one_block_and_dumps_outputs."""
import os

import numpy as np

import bench
from webdgs_amd import synth


class _Buf:
    def __init__(self, a):
        self.a = a

    def read(self, dtype=np.uint32, count=None):
        out = self.a.view(np.uint8).view(dtype)
        return out if count is None else out[:count]


class _FakeTrainer:
    def __init__(self, n, capacity, width, height, seed):
        rng = np.random.default_rng(seed)
        halves = rng.standard_normal((capacity, 60)).astype(np.float16)
        self.n = n
        self.pointCloud = type("PC", (), {})()
        self.pointCloud.gaussian_3d_buffer = _Buf(np.ascontiguousarray(halves[:, :12]).view(np.uint32).ravel())
        self.pointCloud.sh_buffer = _Buf(np.ascontiguousarray(halves[:, 12:]).view(np.uint32).ravel())
        img = _Buf(rng.integers(0, 256, width * height * 4, dtype=np.uint8))
        self.rasterizer = type("R", (), {"getOutputTextureView": lambda self_: img})()

    def getPointCount(self):
        return self.n


def _dump(tmp, cfg, n, capacity, seed=0):
    t = _FakeTrainer(n, capacity, cfg.width, cfg.height, seed)
    bench.dump_outputs(t, cfg, str(tmp))
    return {f[:-4]: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}, t


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    cfg = synth.CONFIGS["c1"]
    out, t = _dump(tmp_path, cfg, 1000, 1200)
    assert sorted(out) == ["gaussians", "gaussians_nonfinite", "image", "sh", "sh_nonfinite"]
    assert all(a.dtype == np.float32 for a in out.values())
    assert out["gaussians"].shape == (1000, 12) and out["sh"].shape == (1000, 48) and out["image"].shape == (cfg.width * cfg.height, 4)
    rows = t.pointCloud.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6)[:1000]
    assert np.array_equal(out["gaussians"], rows.view(np.float16).astype(np.float32)), "rows past the point count are not written"
    assert np.array_equal(out["image"], t.rasterizer.getOutputTextureView().read(np.uint8).reshape(-1, 4).astype(np.float32))
    assert not out["gaussians_nonfinite"].any() and not out["sh_nonfinite"].any()


def test_non_finite_fields_are_zero_in_the_values_and_named_in_the_code(tmp_path):
    """What the reference's densify schedule makes of some Gaussians ("Non-finite Gaussians"): NaN / +-infinity fp16 fields."""
    cfg = synth.CONFIGS["c1"]
    t = _FakeTrainer(100, 100, cfg.width, cfg.height, 0)
    g = t.pointCloud.gaussian_3d_buffer.a.view(np.float16).reshape(-1, 12)
    sh = t.pointCloud.sh_buffer.a.view(np.float16).reshape(-1, 48)
    g[3, 0], g[3, 3], g[50, 9], sh[7, 2] = np.nan, np.inf, -np.inf, np.nan
    bench.dump_outputs(t, cfg, str(tmp_path))
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert all(np.isfinite(a).all() and a.dtype == np.float32 for a in out.values())
    want = np.zeros((100, 12), np.float32)
    want[3, 0], want[3, 3], want[50, 9] = 1, 2, 3
    assert np.array_equal(out["gaussians_nonfinite"], want)
    assert np.argwhere(out["sh_nonfinite"]).tolist() == [[7, 2]] and out["sh_nonfinite"][7, 2] == 1
    assert out["gaussians"][3, 0] == out["gaussians"][3, 3] == out["gaussians"][50, 9] == out["sh"][7, 2] == 0
    finite = want == 0
    assert np.array_equal(out["gaussians"][finite], g.astype(np.float32)[finite])


def test_large_outputs_are_the_same_seeded_sample_within_64_mb(tmp_path):
    cfg = synth.CONFIGS["c5"]
    n = 200_000  # (enough rows to be sampled; the image is c5's full 3840x2160)
    a, _ = _dump(tmp_path / "a", cfg, n, n)
    b, _ = _dump(tmp_path / "b", cfg, n, n)
    assert a["gaussians"].shape == a["gaussians_nonfinite"].shape == (bench.SAMPLE_ROWS, 12) and a["image"].shape == (bench.SAMPLE_PIXELS, 4)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: the same inputs must give the same dump"
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20, total
    # the rows kept do not depend on the data: another cloud of the same size is sampled at the same rows
    c, t = _dump(tmp_path / "c", cfg, n, n, seed=1)
    rows = t.pointCloud.gaussian_3d_buffer.read(np.uint32).reshape(-1, 6).view(np.float16).astype(np.float32)
    assert np.array_equal(c["gaussians"], rows[bench._sample(n, bench.SAMPLE_ROWS)])


def test_plain_run_times_one_block_and_full_keeps_the_repeated_blocks():
    plain, full = bench.parse_args(["--steps", "7"]), bench.parse_args(["--steps", "7", "--full"])
    assert plain.steps == 7 and plain.min_seconds == 0.0 and not plain.full and plain.dump_outputs is None
    assert full.full and full.min_seconds == 1.0
    assert bench.parse_args(["--min-seconds", "0.3"]).min_seconds == 0.3
    assert bench.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"
