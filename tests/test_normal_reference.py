"""The float64 restatement of the normal maps (tests/normal64.py) against what it claims to restate: the per-Gaussian normal is the minor eigenvector of
the covariance the projection builds, the packed word round-trips within the snorm16 step, the compositing is depth64's walk, the depth-normal stencil
returns an analytic plane's normal, and the exclusion mask of the GPU tests (near_flip) stays small.  No GPU: this protects the yardstick the GPU normal
tests measure against."""
import functools
import math

import numpy as np
import pytest

from webdgs_amd import ops, synth

import harness
import normal64 as n64
from test_depth_reference import MASK_CAP, SCENES, reference, scene_config

FLIP_CAP = 0.005           # share of a scene's Gaussians near_flip may hold
WALKED = ["big-splats", "sparse", "odd-size"]   # the CPU scenes whose lists are walked here (three walks each: the small ones)


@functools.lru_cache(maxsize=None)
def scene_normals(name):
    cfg = scene_config(name)
    g, sh, cam = harness.scene(cfg)
    return cfg, g, cam, n64.gaussian_normals64(g, cam)


@pytest.mark.parametrize("name", list(SCENES))
def test_normal_is_the_minor_eigenvector_of_the_covariance(name):
    cfg, g, cam, nrm = scene_normals(name)
    h = n64.halves(g)
    q, s = h[:, 4:8], np.exp(h[:, 8:11])
    assert nrm["valid"].all()
    qn = np.linalg.norm(q, axis=1)
    assert np.abs(qn - 1).max() < 1e-3, "the scenes' fp16 quaternions are unit to the fp16 rounding"
    # (a) for the unit quaternion the row is an exact eigenvector for s_k^2 -- and the column is not
    qh = q / qn[:, None]
    C = n64.covariance64(qh, s)
    smax2 = (s.max(axis=1) ** 2)
    sk2 = np.take_along_axis(s, nrm["k"][:, None], axis=1)[:, 0] ** 2
    row = nrm["world"]
    res_row = np.linalg.norm(np.einsum("nij,nj->ni", C, row) - sk2[:, None] * row, axis=1) / smax2
    col = n64.quat_to_rows(qh)[np.arange(len(q)), :, nrm["k"]]
    res_col = np.linalg.norm(np.einsum("nij,nj->ni", C, col) - sk2[:, None] * col, axis=1) / smax2
    print(f"{name}: row residual {res_row.max():.2e}, column residual up to {res_col.max():.2f}")
    assert res_row.max() <= 1e-14 and res_col.max() > 0.01, "it is the row of R, not the column"
    # (b) for the fp16 quaternion as stored (the covariance the projection builds): the minor eigenvector by eigh, up to sign, within the
    # Davis-Kahan bound sin(theta) <= 2 |E| / gap (Yu, Wang, Samworth 2015), E = cov(q) - cov(q / |q|), gap = s_mid^2 - s_min^2 of the unit one
    Cq = n64.covariance64(q, s)
    E = np.linalg.norm(Cq - C, ord=2, axis=(1, 2))
    s2 = np.sort(s * s, axis=1)
    gap = s2[:, 1] - s2[:, 0]
    evec = np.linalg.eigh(Cq)[1][:, :, 0]
    sin_theta = np.linalg.norm(np.cross(evec, row), axis=1)
    with np.errstate(divide="ignore"):
        bound = np.minimum(1.0, 2.0 * E / gap + 1e-9)
    # |E| itself follows from the distance to unit norm: R(q) = R^ + d (R^ - I), d = |q|^2 - 1, so |E| <= s_max^2 (4 |d| + 4 d^2)
    d = np.abs(qn * qn - 1)
    assert np.all(E <= smax2 * (4 * d + 4 * d * d) * (1 + 1e-9) + 1e-18)
    sharp = bound < 0.1
    print(f"{name}: worst sin(angle to eigh) / bound = {np.max(sin_theta / bound):.3f}; the bound is below 0.1 on {sharp.mean():.1%}, worst angle there {sin_theta[sharp].max():.2e}")
    assert np.all(sin_theta <= bound)
    assert sharp.mean() > 0.5


def test_ties_go_to_the_lowest_index_and_flip_follows_the_definition():
    f16 = lambda v: np.float16(v).view(np.uint16)   # noqa: E731
    g = np.zeros((5, 12), np.uint16)
    g[:, 4] = f16(1.0)
    g[:, 0:3] = [f16(1.0), f16(1.0), f16(4.0)]
    for i, ls in enumerate([(-3, -2, -1), (-2, -3, -3), (-3, -3, -3), (-1, -2, -3), (0.0, -0.0, 1.0)]):
        g[i, 8:11] = [f16(v) for v in ls]
    cfg = harness.small_config("c1", num_points=5)
    out = n64.gaussian_normals64(g.view(np.uint32).reshape(5, 6), synth.identity_camera(cfg))
    assert list(out["k"]) == [0, 1, 0, 2, 0]
    assert list(out["tie"]) == [False, True, True, False, True]
    want = -np.eye(3)[[0, 1, 0, 2, 0]]      # p = (1, 1, 4): every axis faces away and is turned round
    assert np.array_equal(out["normal"], want)
    words = n64.encode64(out["normal"])
    assert np.array_equal(n64.decode64(words), want) and np.array_equal(ops.decodeNormals(words).astype(np.float64), want)


def test_encode_decode_round_trip():
    rng = np.random.default_rng(12)
    v = rng.standard_normal((200_000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    t = np.linspace(0, 2 * math.pi, 4001)
    edge = np.stack([np.cos(t), np.sin(t), np.zeros_like(t)], axis=1)                       # the fold line
    near = edge + np.array([0, 0, 1e-7]) * np.sign(np.sin(7 * t))[:, None]
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    diag = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) / math.sqrt(3)
    scene = scene_normals("c1")[3]["normal"]
    allv = np.concatenate([v, edge, near / np.linalg.norm(near, axis=1)[:, None], axes, diag, scene])
    words = n64.encode64(allv)
    assert not np.any(words == np.uint32(n64.NO_NORMAL)), "the encoder never produces the no-normal word"
    lo, hi = (words & 0xFFFF).astype(np.uint16).view(np.int16), (words >> 16).astype(np.uint16).view(np.int16)
    assert lo.min() >= -32767 and hi.min() >= -32767
    back = n64.decode64(words)
    err = np.linalg.norm(back - allv, axis=1)
    print(f"round trip: worst error {err.max():.3e} = {err.max() / n64.ROUND_TRIP:.3f} of the bound sqrt(18) / 2 / 32767 = {n64.ROUND_TRIP:.3e}")
    assert err.max() <= n64.ROUND_TRIP
    assert np.array_equal(n64.decode64(n64.encode64(axes)), axes), "the axes are exact"
    # the f32 decode of ops.decodeNormals (the kernel's, operation by operation) against the float64 one
    f32 = ops.decodeNormals(words)
    assert f32.dtype == np.float32 and np.abs(f32.astype(np.float64) - back).max() <= 12 * n64.U
    assert np.array_equal(n64.decode64(np.array([n64.NO_NORMAL], np.uint32)), np.zeros((1, 3)))
    assert np.array_equal(ops.decodeNormals(np.array([n64.NO_NORMAL], np.uint32)), np.zeros((1, 3), np.float32))


@pytest.mark.parametrize("name", list(SCENES))
def test_flip_mask_and_ties_are_rare(name):
    cfg, g, cam, nrm = scene_normals(name)
    near_flip = np.abs(nrm["facing"]) < n64.NEAR_FLIP
    print(f"{name}: near_flip {near_flip.mean():.4%} of {len(near_flip)} Gaussians, ties of the smallest log-scale {nrm['tie'].mean():.4%}")
    assert near_flip.mean() <= FLIP_CAP
    assert np.all(np.sum(nrm["normal"] * nrm["unflipped"], axis=1)[~near_flip] * np.sign(-nrm["facing"][~near_flip]) > 0.999999)
    h = n64.halves(g)[:, 8:11]
    assert np.array_equal(nrm["k"], np.argmin(h, axis=1)), "argmin takes the first of equal values: the lowest index"
    # camera-facing: n . p <= 0 everywhere
    view = cam.astype(np.float64)[0:16].reshape(4, 4).T
    p = n64.halves(g)[:, 0:3] @ view[:3, :3].T + view[:3, 3]
    assert np.all(np.sum(nrm["normal"] * p, axis=1) <= 0)


@pytest.mark.parametrize("name", WALKED)
def test_compositing_is_depth64s_walk(name):
    cfg, ref, (A, D, M, near_sat, near_half, stats) = reference(name)
    _, g, cam, nrm = scene_normals(name)
    n32 = ops.decodeNormals(n64.encode64(nrm["normal"]))
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    A2, N, near_sat2, n_active = n64.composite64(st, ti, ref, n32)
    assert np.array_equal(A2, A) and np.array_equal(near_sat2, near_sat) and np.array_equal(n_active, stats["n_active"])
    assert near_sat.mean() <= MASK_CAP
    length = np.linalg.norm(N, axis=2)
    assert np.all(length <= A * (1 + 4 * n64.U) + 1e-300), "|N| <= A: a convex combination of unit vectors (unit to the f32 decode's 3u), times A"
    assert np.all(N[n_active == 0] == 0)
    # a Gaussian without a normal adds its weight and nothing else: drop every second normal
    n_half = n32.copy()
    n_half[::2] = 0
    A3, N3, _, _ = n64.composite64(st, ti, ref, n_half)
    assert np.array_equal(A3, A) and np.all(np.linalg.norm(N3, axis=2) <= A * (1 + 4 * n64.U) + 1e-300)
    # presentation ties on this image
    rgb, v = n64.normal_to_rgba8_64(np.concatenate([N, A[..., None]], axis=2).astype(np.float32))
    # (per colour byte: a window of 2e-3 around each of 255 ties holds 0.2 % of uniformly spread values, so 0.6 % of the pixels have one in some channel)
    ties = np.abs((v - np.floor(v)) - 0.5) < 1e-3
    print(f"{name}: presentation tie share {ties.mean():.4%} of the colour bytes")
    assert ties.mean() <= MASK_CAP
    assert np.all(rgb[n_active == 0] == 0)


def test_two_gaussians_on_one_pixel():
    from oracle import oracle as orc
    from test_depth_reference import _two_gaussians
    cfg, g, sh, cam = _two_gaussians(0.0, 3.0)
    gh = g.view(np.uint16).reshape(-1, 12).copy()
    f16 = lambda v: np.float16(v).view(np.uint16)   # noqa: E731
    gh[0, 8:11] = [f16(-3.0), f16(-2.0), f16(-2.0)]    # shortest axis x -> (+-1, 0, 0)
    gh[1, 8:11] = [f16(-2.0), f16(-2.0), f16(-3.0)]    # shortest axis z -> (0, 0, -1)
    g = gh.view(np.uint32).reshape(-1, 6)
    ref = orc.forward(g, sh, cam, synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0))
    nrm = n64.gaussian_normals64(g, cam)
    assert np.array_equal(nrm["normal"], np.array([[-1.0, 0, 0], [0, 0, -1.0]]))
    n32 = ops.decodeNormals(n64.encode64(nrm["normal"]))
    A, N, _, n_active = n64.composite64(synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0), ref, n32)
    stored = ref["splats"].view(np.uint16).reshape(-1, 12)[:, 11].view(np.float16).astype(np.float64)
    w1, w2 = stored[0], stored[1] * (1.0 - stored[0])
    assert n_active[32, 32] == 2
    assert A[32, 32] == pytest.approx(w1 + w2, rel=1e-15)
    assert N[32, 32] == pytest.approx(np.array([-w1, 0.0, -w2]), rel=1e-14, abs=1e-300)


def _plane_depth(width, height, cam, normal, dist, dtype=np.float64):
    """Depth image of the view-space plane n . X = dist under the camera's projection (pixel centres), and the unit normal turned toward the camera."""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    p00, p11 = float(cam[32]), float(cam[37])
    jj, ii = np.mgrid[0:height, 0:width]
    rx, ry = (2.0 * (ii + 0.5) / width - 1.0) / p00, (1.0 - 2.0 * (jj + 0.5) / height) / p11
    z = dist / (n[0] * rx + n[1] * ry + n[2])
    facing = -n if dist > 0 else n    # n . X = dist > 0: n points away from the origin
    return z.astype(dtype), facing


PLANES = [((0.3, -0.2, 1.0), 4.0), ((-0.5, 0.4, 1.0), 6.0), ((0.0, 0.0, 1.0), 3.0), ((0.6, 0.6, -1.0), -5.0)]


@pytest.mark.parametrize("normal,dist", PLANES)
def test_depth_normals_of_an_analytic_plane(normal, dist):
    cfg = harness.small_config("c1", num_points=1, width=97, height=61)
    cam = synth.identity_camera(cfg)
    z, want = _plane_depth(cfg.width, cfg.height, cam, normal, dist)
    assert z.min() > 0
    dn = n64.depth_normals64(z, cam[32], cam[37])
    inner = np.zeros(z.shape, bool)
    inner[1:-1, 1:-1] = True
    assert np.array_equal(dn["valid"], inner), "borders have no normal"
    assert np.all(dn["normal"][~inner] == 0)
    err = np.abs(dn["normal"][inner] - want).max()
    print(f"plane {normal}: worst |n - analytic| = {err:.2e}")
    assert err <= 1e-6
    # holes: a pixel without depth takes its four neighbours' normals with it
    holes = z.copy()
    holes[20, 30], holes[40, 50], holes[10, 10], holes[30, 60] = 0.0, -1.0, np.nan, np.inf
    dh = n64.depth_normals64(holes, cam[32], cam[37])
    for (j, i) in ((20, 30), (40, 50), (10, 10), (30, 60)):
        for dj, di in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            assert not dh["valid"][j + dj, i + di] and np.all(dh["normal"][j + dj, i + di] == 0)
    assert dh["valid"].sum() == inner.sum() - 20
    # the f32 bound the GPU test uses is far below the tolerance asked of the kernel's users
    assert n64.depth_normals_f32_bound(dn)[inner].max() < 1e-3


def test_agreement_of_a_plane_with_itself_is_zero():
    cfg = harness.small_config("c1", num_points=1, width=97, height=61)
    cam = synth.identity_camera(cfg)
    z, want = _plane_depth(cfg.width, cfg.height, cam, (0.3, -0.2, 1.0), 4.0)
    dn = n64.depth_normals64(z, cam[32], cam[37])
    dimg = np.concatenate([dn["normal"], dn["valid"][..., None].astype(np.float64)], axis=2).astype(np.float32)
    A = np.full(z.shape, 0.75)
    A[:, :10] = 0.25    # below one half: not counted
    comp = np.concatenate([want[None, None, :] * A[..., None], A[..., None]], axis=2).astype(np.float32)
    e, a, cnt = n64.agreement64(comp, dimg)
    assert cnt == (cfg.height - 2) * (cfg.width - 11) and a == cnt * int(0.75 * 2 ** 24)
    assert e <= cnt * 2, "1 - cos of a direction with its own f32 rounding: a unit or two of 2^-24"
    flipped = comp * np.array([-1, -1, -1, 1], np.float32)
    e2, _, _ = n64.agreement64(flipped, dimg)
    assert abs(e2 / a - 2.0) < 1e-6
