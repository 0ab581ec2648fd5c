#!/usr/bin/env python3
"""What the tile-list walkers off the training path write, as digests: per scene the sha256 of the three depth images and of the raw contribution
records after one forward, rasterize, encodeDepth (all kinds) and encodeContribution.

    python scripts/walk_outputs_digest.py                (needs an MI355X)

Both outputs are integer or per-pixel-sequential results, so two builds of the library that perform the same operations print the same listing, line
for line: run once with WDGS_LIB_PATH pointing at another build (scripts/build_prev_lib.sh) and once without, each in a process of its own, and diff.
The scenes are the test suite's: test_depth_reference.SCENES uncapped and with compat_caps, test_gpu_depth._special_scenes() (non-finite tiles and lists
past 4 096 entries), test_gpu_nan.chunk_edge_scene() (lists that end at the walk's chunk edges).
"""
import hashlib
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]


def main():
    from webdgs_amd import ops
    import harness
    from test_depth_reference import SCENES, scene_config
    from test_gpu_depth import ALL, _special_scenes
    from test_gpu_nan import chunk_edge_scene

    def scenes():
        for name in SCENES:
            cfg = scene_config(name)
            for compat in (False, True):
                yield (f"{name} {'compatCaps' if compat else 'uncapped'}", cfg) + harness.scene(cfg) + (compat,)
        for what, cfg, g, sh, cam in _special_scenes():
            yield what, cfg, g, sh, cam, False
        yield ("chunk edges",) + chunk_edge_scene() + (False,)

    dev = ops.HipDevice(0)
    for what, cfg, g, sh, cam, compat in scenes():
        pipe = harness.HipPipeline(dev, cfg, g, sh, cam, compat_caps=compat)
        buf = ops.createContributionBuffer(dev, cfg.num_points)
        pipe.forward()
        pipe.rast.encodeDepth(None, ALL)
        pipe.rast.encodeContribution(None, buf)
        dev.synchronize()
        digests = [hashlib.sha256(pipe.rast.getDepthTextureView(k).read(np.uint32).tobytes()).hexdigest()[:16] for k in ALL]
        digests.append(hashlib.sha256(buf.read(np.uint8, 16 * cfg.num_points).tobytes()).hexdigest()[:16])
        print(f"{what:32s} " + " ".join(f"{k} {d}" for k, d in zip(ALL + ("contribution",), digests)), flush=True)
        buf.destroy()
        pipe.destroy()
    dev.destroy()


if __name__ == "__main__":
    main()
