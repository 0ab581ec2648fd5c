#!/usr/bin/env python3
"""What the image-window kernels write, as digests: per image size and kind the sha256 of the SSIM map and the 64 bits of its mean (csrc/ssim.hip), the
sha256 of the loss image in dssim_mode="gaussian" at the three lambda settings of tests/test_gpu_dssim_loss.py (csrc/dssim.hip), and of the loss image in
reference mode at the first of them (csrc/loss.hip).

    python scripts/ssim_outputs_digest.py                (needs an MI355X)

No kernel here uses an atomic, and each value is one fixed sequence of operations, so two builds of the library that perform the same operations print
the same listing, line for line: run once with WDGS_LIB_PATH pointing at another build (scripts/build_prev_lib.sh) and once without, each in a process
of its own, and diff.  The images are the test suite's: test_gpu_eval.SIZES + EDGE_SIZES, every kind of KINDS, with the tests' seeds.
"""
import hashlib
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]


def _sha(buf, dtype):
    return hashlib.sha256(buf.read(dtype).tobytes()).hexdigest()[:16]


def main():
    from webdgs_amd import ops
    from test_gpu_dssim_loss import LAMBDAS, _lam, _pass
    from test_gpu_eval import EDGE_SIZES, KINDS, SIZES, _pair

    dev = ops.HipDevice(0)
    for w, h in SIZES + EDGE_SIZES:
        passes = {mode: _pass(dev, w, h, dssim_mode=mode) for mode in ("gaussian", "reference")}
        mbuf = dev.createBuffer(12 * w * h, "ssim map")
        for k, kind in enumerate(KINDS):
            a, b = _pair(kind, w, h, seed=w * 7919 + h * 31 + k)
            ba, bb = dev.bufferFrom(a), dev.bufferFrom(b)
            mean = ops.imageSSIM(dev, ba, bb, w, h, mbuf)
            out = [f"map {_sha(mbuf, np.uint32)}", f"mean {np.float64(mean).view(np.uint64).item():016x}"]
            for mode, lams in (("gaussian", LAMBDAS), ("reference", LAMBDAS[:1])):
                for lam in lams:
                    passes[mode].setTrainingConfig(_lam(lam))
                    passes[mode].computeLossOnly(None, ba, bb)
                    out.append(f"{mode}{lam} {_sha(passes[mode].getLossTextureView(), np.uint32)}")
            print(f"{w}x{h} {kind:10s} " + " ".join(out), flush=True)
            ba.destroy()
            bb.destroy()
        mbuf.destroy()
        for p in passes.values():
            p.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
