"""The camera zoo: poses the synthetic builders (synth.identity_camera, synth.circle_cameras) never produce -- rolled, steep, behind, inside the cloud,
far away, looking away, and a hand's breadth from one Gaussian.  Under the identity every product with a view-matrix entry is exact and the 3x3 is its
own transpose; a circle camera has view[0][1] == 0, no roll, and every Gaussian at view depth >= 2.  The kernels that read the camera block
(project.hip: project_one, backward.hip: the geometry kernels, normal.hip) are compared under these poses by tests/test_gpu_cameras.py; that every
case reaches what it is there for is pinned on the CPU by tests/test_camera_zoo_reference.py.  A plain helper module: no fixtures, every input generated."""
import functools
import math

import numpy as np

from webdgs_amd import synth

import harness


def look_at(position, target, roll_deg=0.0, up=(0.0, 1.0, 0.0)):
    """4x4 world->view matrix (row-major), built as synth.circle_cameras builds it (f = normalize(target - position), x = normalize(cross(up, f)),
    y = cross(f, x)), then rolled about the optical axis: x' = cos r x + sin r y, y' = -sin r x + cos r y.  Rows (x', y', f), translation -R position."""
    c = np.asarray(position, np.float64)
    f = np.asarray(target, np.float64) - c
    f = f / np.linalg.norm(f)
    x = np.cross(np.asarray(up, np.float64), f)
    x = x / np.linalg.norm(x)
    y = np.cross(f, x)
    r = math.radians(roll_deg)
    xr, yr = math.cos(r) * x + math.sin(r) * y, -math.sin(r) * x + math.cos(r) * y
    rot = np.stack([xr, yr, f], axis=0)
    view = np.eye(4)
    view[:3, :3] = rot
    view[:3, 3] = -rot @ c
    return view


ZOO_CFG = harness.small_config("c3", num_points=6000, width=160, height=112, s0=0.01, fy=150.0)   # SH degree 3, 10 x 7 tiles, a ragged last row

# name -> (position, target, roll in degrees, up); `close` is placed relative to a Gaussian of the scene (poses())
_FIXED = {
    "roll37": ((0.7, 0.4, 0.0), (0.0, 0.0, 6.0), 37.0, (0.0, 1.0, 0.0)),
    "roll90": ((0.7, -0.4, 0.0), (0.2, 0.1, 6.0), 90.0, (0.0, 1.0, 0.0)),
    "roll180": ((-0.6, 0.5, 0.0), (0.0, 0.0, 6.0), 180.0, (0.0, 1.0, 0.0)),
    "side": ((9.0, 1.0, 5.0), (0.0, 0.0, 6.0), -20.0, (0.0, 1.0, 0.0)),
    "behind": ((1.0, -1.5, 13.0), (0.0, 0.0, 6.0), 63.0, (0.0, 1.0, 0.0)),
    "below": ((0.5, 7.0, 4.0), (0.0, 0.0, 6.0), 15.0, (0.0, 0.0, 1.0)),
    "inside": ((0.1, 0.1, 4.0), (3.0, 1.0, 5.0), 30.0, (0.0, 1.0, 0.0)),
    "far": ((3.0, -2.0, -50.0), (0.0, 0.0, 6.0), -50.0, (0.0, 1.0, 0.0)),
    "away": ((0.0, 0.0, 0.0), (0.3, 0.2, -6.0), 10.0, (0.0, 1.0, 0.0)),
}
CLOSE_TO = 123        # `close` sits 2.3 cm in front of this Gaussian's fp16 position
NAMES = list(_FIXED) + ["close"]
BATCH_NAMES = ["roll37", "roll90", "roll180", "side", "behind", "below", "inside", "far"]   # the view-batched test's dataset, in this order


@functools.lru_cache(maxsize=None)
def scene():
    """(gaussians, sh) of ZOO_CFG.  Shared: callers copy before they write."""
    g, sh = synth.make_gaussians(ZOO_CFG)
    g.setflags(write=False)
    sh.setflags(write=False)
    return g, sh


@functools.lru_cache(maxsize=None)
def poses():
    """name -> (position, target, roll, up), `close` included."""
    g, _ = scene()
    p = g.view(np.float16).reshape(-1, 12)[CLOSE_TO, 0:3].astype(np.float64)
    out = dict(_FIXED)
    out["close"] = (tuple(p - np.array([0.01, -0.005, 0.02])), tuple(p + np.array([0.2, 0.1, 1.0])), 25.0, (0.0, 1.0, 0.0))
    return out


def view_matrix(name):
    position, target, roll, up = poses()[name]
    return look_at(position, target, roll, up)


@functools.lru_cache(maxsize=None)
def _camera(name):
    cam = synth.camera_block(view_matrix(name), ZOO_CFG.width, ZOO_CFG.height, ZOO_CFG.fy)
    cam.setflags(write=False)
    return cam


def camera(name):
    """The 68-float camera block of a zoo camera at ZOO_CFG's viewport."""
    return _camera(name)


def settings():
    return synth.render_settings(ZOO_CFG), synth.tile_info(ZOO_CFG.width, ZOO_CFG.height, 0)


@functools.lru_cache(maxsize=None)
def target(name):
    """The oracle's render of the target scene (synth.make_target_scene) under a zoo camera: what the zoo trains towards."""
    from oracle import oracle as orc
    g, sh = scene()
    tg, tsh = synth.make_target_scene(g, sh)
    st, ti = settings()
    img = orc.forward(tg, tsh, camera(name), st, ti)["rgba8"].copy()
    img.setflags(write=False)
    return img
