"""CPU: implementation-independent evidence for the oracle.

The reference ships no test vector, so the C++ oracle -- against which every GPU result is compared bit for bit -- is
"parity unpinned".  What CAN be pinned is that the oracle computes what the mathematics says.  ``tests/indep64.py`` restates the
per-Gaussian mathematics from the textbook formulas in float64 numpy (no code shared with ``oracle/``, ``wgslm.h`` or the kernels);
this file compares:

  (a) K1  projection, conic, SnugBox extents, SH colour (degrees 0..3), depth key, tile counts           -- test_k1_*
  (b) K17 the chain rule to position / log-scale / quaternion / raw opacity, against central differences of the float64 forward;
          the reference's K17 deviates from the true gradient in exactly the places named in the test                -- test_k17_*
  (c) K18 Adam without bias correction, quaternion renormalisation, visibility skip                                 -- test_adam_*
  (d) K26-K30 densify decisions, capacity rule, offsets, clone / split children                                     -- test_densify_*
  (e) K15 loss gradient (L1 / L2 / DSSIM with 5x5 box statistics)                                                   -- test_k15_*
  (f) K21-K23 metric map, K24 metric counts, K31 ground-truth downsample                                            -- test_k21_*, test_k24_*, test_k31_*

K14 / K16 have their float64 checks in tests/test_oracle_golden.py (re-composite, finite differences of the composite)."""
import numpy as np
import pytest

from webdgs_amd import synth

import harness
import indep64 as ind
from densifycases import _densify_children_fp64, _rand01  # noqa: F401


def _scene(base="c1", n=None, w=None, h=None, sh_deg=None, s0=None, view=None):
    cfg = harness.small_config(base, num_points=n, width=w, height=h, sh_deg=sh_deg, s0=s0)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.identity_camera(cfg) if view is None else synth.circle_cameras(cfg, 8)[view]
    return cfg, g, sh, cam


# ----------------------------------------------------------------------------------------------------------------- (a) K1
@pytest.mark.parametrize("case", [dict(base="c1"), dict(base="c1", view=3), dict(base="c2", n=6000, sh_deg=1, view=5), dict(base="c2", n=6000, w=320, h=240, sh_deg=2, view=1),
                                  dict(base="c3", n=8000, w=480, h=272, sh_deg=3, view=6, s0=0.01)],
                         ids=["c1-identity", "c1-rotated", "sh1", "sh2", "sh3"])
def test_k1_projection_extents_colour_and_tile_counts(orc, case):
    check_k1(orc, *_scene(**case))


def check_k1(orc, cfg, g, sh, cam, population_floor=0.3):
    """K1 of the oracle against the float64 restatement under the camera given.  `population_floor`: the share of the cloud that must be visible to
    both (a condition on the input, not a tolerance: a camera inside the cloud sees less of it)."""
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    splats, depths, counts, _ = orc.project_count(g, sh, cam, st, ti)
    got = splats.view(np.float16).reshape(-1, 12)           # ndc.xy | extent.xy | conic.xy | conic.z, 0 | r, g | b, sigma(o)
    gs, cp = ind.unpack_gaussians(g), ind.camera_parts(cam)
    pr = ind.project(gs, cp)
    tb = ind.tile_boxes(pr, cp)
    col = ind.colour(gs, ind.unpack_sh(sh), cp, cfg.sh_deg)

    # visibility and tile counts: identical except where a float32 and a float64 evaluation of the same number fall on different sides
    # of an fp16 rounding boundary or of a tile edge (documented ties): a handful in 10 k at most, each off by one tile row / column
    vis_o = counts > 0
    assert (vis_o != tb["visible"]).sum() <= max(2, vis_o.size // 3000), ((vis_o != tb["visible"]).sum(), vis_o.size)
    both = vis_o & tb["visible"]
    assert both.sum() > population_floor * vis_o.size, (both.sum(), vis_o.size)
    differ = np.flatnonzero(both & (counts != tb["count"]))
    assert differ.size <= max(3, both.sum() // 1500), (differ.size, both.sum())
    for i in differ:  # each explained by the stored fp16 centre / extent being one ulp away from the float64 value's rounding
        ulps = max(ind.f16_ulp_distance(got[i, 0:4].view(np.uint16), ind.f16_bits(np.concatenate([tb["ndc16"][i], tb["ext16"][i]]))).max(), 0)
        assert ulps <= 1 or abs(int(counts[i]) - int(tb["count"][i])) <= max(tb["tile_max"][i] - tb["tile_min"][i] + 1), (i, ulps, counts[i], tb["count"][i])

    # stored fp16 fields vs the float64 value rounded to fp16: within one unit in the last place, and mostly identical
    want = np.concatenate([np.clip(pr["ndc"][:, :2], -60000, 60000), pr["extent_capped"], pr["conic"], np.zeros((g.shape[0], 1)),
                           np.clip(col, 0, 1), np.clip(pr["sigma"], 0, 1)[:, None]], 1)
    d = ind.f16_ulp_distance(got[both].view(np.uint16), ind.f16_bits(want[both]))
    names = ["ndc.x", "ndc.y", "extent.x", "extent.y", "conic.x", "conic.y", "conic.z", "pad", "r", "g", "b", "sigma"]
    # (the off-diagonal conic term is a difference of products: where it all but cancels, one fp16 ulp of a number 1e-5 of the diagonal
    # says nothing, and the float32 result is judged against the diagonal's scale instead)
    abs_err = np.abs(got[both].astype(np.float64) - want[both])
    slack = np.zeros_like(abs_err)
    slack[:, 5] = 1e-5 * np.sqrt(np.abs(want[both][:, 4] * want[both][:, 6]))
    for j, name in enumerate(names):
        bad = (d[:, j] > 1) & (abs_err[:, j] > slack[:, j])
        assert not bad.any(), (name, int(d[:, j].max()), int(np.argmax(bad)))
        assert (d[:, j] == 0).mean() > 0.97, (name, float((d[:, j] == 0).mean()))

    # depth key: top 16 bits of the ordered view depth (7 mantissa bits: a float32 / float64 disagreement is a 1-in-10^5 event)
    key = ind.depth_key16(pr["t"][:, 2])
    assert ((depths[both] >> 16) != key[both]).sum() <= 1


def test_k1_real_sh_basis_is_the_scipy_one():
    """The colour model's basis functions are the real spherical harmonics (Condon-Shortley phase kept), orthonormal on the sphere:
    checked by quadrature, so the SH constants the oracle multiplies by are pinned by scipy, not by a transcription."""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = ind.real_sh_basis(d, 3)
    gram = 4 * np.pi * (Y.T @ Y) / d.shape[0]           # Monte-Carlo <Y_j, Y_k> over the sphere
    assert np.abs(gram - np.eye(16)).max() < 0.03
    # l = 1 in the colour model's order and sign: -y, +z, -x (times sqrt(3 / 4 pi))
    c1 = np.sqrt(3 / (4 * np.pi))
    assert np.allclose(Y[:, 1:4], np.stack([-c1 * d[:, 1], c1 * d[:, 2], -c1 * d[:, 0]], 1), atol=1e-12)


# ----------------------------------------------------------------------------------------------------------------- (b) K17
def _k17_scene(view):
    cfg = harness.small_config("c2", num_points=4000, width=640, height=480, sh_deg=0, s0=0.02)
    g, sh = synth.make_gaussians(cfg)
    cam = synth.circle_cameras(cfg, 8, radius=2.5)[view]           # a clearly rotated view (Q10 needs view3x3 != its transpose)
    return cfg, g, sh, cam


def _k17_case(orc, cfg, g, sh, cam, n=400, seed=0):
    """Visible, well-conditioned Gaussians under a rotated camera, random cotangents for (pixel centre, conic, sigma(opacity)) given to
    K17 as exact fixed-point accumulators, and F(params) = <cotangent, float64 forward(params)> whose gradient K17 claims to be."""
    gs, cp = ind.unpack_gaussians(g), ind.camera_parts(cam)
    pr = ind.project(gs, cp)
    tb = ind.tile_boxes(pr, cp)
    lim = 1.2 * np.array([0.5 * cp["width"] / cp["fx"], 0.5 * cp["height"] / cp["fy"]])
    ok = tb["visible"] & (np.abs(pr["t"][:, 0] / pr["t"][:, 2]) < lim[0]) & (np.abs(pr["t"][:, 1] / pr["t"][:, 2]) < lim[1]) & (pr["extent"].max(1) < 100.0)
    pick = np.flatnonzero(ok)[:n]
    assert pick.size >= 200
    g = np.ascontiguousarray(g[pick])
    rng = np.random.default_rng(seed)
    m = pick.size
    gm = rng.integers(-3_000_000, 3_000_000, (m, 2)).astype(np.int32)       # dF / d(pixel centre), x 1e6
    gc = np.zeros((m, 4), np.int32)
    gc[:, [0, 1, 3]] = rng.integers(-40_000_000, 40_000_000, (m, 3))         # dF / d(conic.x, conic.y, conic.z), x 1e6 (slot 2 unused)
    go = rng.integers(-2_000_000, 2_000_000, m).astype(np.int32)            # dF / d(sigma(opacity_raw)), x 1e6
    gcol = rng.integers(-1_000_000, 1_000_000, (m, 3)).astype(np.int32)
    st = synth.render_settings(cfg)
    st[5] = 0.0
    return cfg, g, cam, st, gm, gc, go, gcol


def _k17_fd(g, cam, gm, gc, go):
    """Central differences of F in float64, one parameter of every Gaussian at a time (F_i depends on Gaussian i only)."""
    cp = ind.camera_parts(cam)
    base = ind.unpack_gaussians(g)
    wm, wc, wo = gm / 1e6, gc[:, [0, 1, 3]] / 1e6, go / 1e6

    def F(gs):
        pr = ind.project(gs, cp)
        return (wm * pr["px"]).sum(1) + (wc * pr["conic"]).sum(1) + wo * pr["sigma"]

    out = {}
    for key, width in (("pos", 3), ("opacity_raw", 1), ("quat", 4), ("log_scale", 3)):
        cols = []
        for j in range(width):
            eps = 1e-5
            hi, lo = {k: v.copy() for k, v in base.items()}, {k: v.copy() for k, v in base.items()}
            if width == 1:
                hi[key] = hi[key] + eps; lo[key] = lo[key] - eps
            else:
                hi[key][:, j] += eps; lo[key][:, j] -= eps
            cols.append((F(hi) - F(lo)) / (2 * eps))
        out[key] = np.stack(cols, 1)
    return out


def _k17_oracle(orc, g, cam, st, gm, gc, go, gcol, flags):
    orc.set_k17_fix(flags)
    try:
        grads = orc.geometry_backward(cam, st, g, np.ascontiguousarray(gm.reshape(-1)), np.ascontiguousarray(gc.reshape(-1)), go, np.ascontiguousarray(gcol.reshape(-1)))
    finally:
        orc.set_k17_fix(0)
    h = grads.view(np.float16).reshape(-1, 16).astype(np.float64)
    return dict(pos=h[:, 0:3], opacity_raw=h[:, 3:4], quat=h[:, 4:8], log_scale=h[:, 8:11], colour=h[:, 12:15])


def _rel(got, ref):
    """Worst per-Gaussian error relative to that Gaussian's gradient norm (floored at 1 % of the median norm)."""
    nrm = np.linalg.norm(ref, axis=1)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(nrm, 0.01 * np.median(nrm))).max())


@pytest.mark.parametrize("view", [1, 4, 6])
def test_k17_with_its_three_deviations_undone_is_the_true_gradient(orc, view):
    """The reference's K17, as restated by the oracle, with Q10, Q11 and Q23 switched off (oracle_backward.cpp: orc_set_k17_fix) equals
    the float64 finite-difference gradient of the float64 forward to fp16 output precision -- for position, raw opacity, quaternion and
    log-scale.  So these three are the ONLY places where the restated chain rule departs from the true gradient; everything else in
    K17 (Jacobian, clamp masks, quaternion and scale chain, sigmoid) is read and evaluated correctly."""
    check_k17(orc, *_k17_scene(view))


def check_k17(orc, cfg, g, sh, cam):
    """K17 with its three deviations undone against float64 central differences, on the visible, well-conditioned Gaussians of the camera given."""
    cfg, g, cam, st, gm, gc, go, gcol = _k17_case(orc, cfg, g, sh, cam)
    fd = _k17_fd(g, cam, gm, gc, go)
    got = _k17_oracle(orc, g, cam, st, gm, gc, go, gcol, flags=7)
    for key in ("pos", "opacity_raw", "quat", "log_scale"):
        err = _rel(got[key], fd[key])
        assert err < 3e-3, (key, err)          # fp16 outputs: 2^-11 = 4.9e-4 per component, fp32 arithmetic inside
    # colour passes through K17 unchanged (tiled-backward.wgsl:293-297): the fixed-point sums, rounded to fp16
    assert np.array_equal(got["colour"], ind.f16_round(gcol / 1e6))


@pytest.mark.parametrize("flags,broken", [(0, ("pos", "quat", "log_scale")), (6, ("pos", "quat", "log_scale")), (5, ("pos",)), (3, ("pos", "quat", "log_scale"))],
                         ids=["reference", "only-Q10-left", "only-Q11-left", "only-Q23-left"])
def test_k17_each_deviation_is_real(orc, flags, broken):
    """Leaving any one of the three in place breaks the agreement (so each switch undoes a real deviation, and the reference's K17 --
    flags 0, what the product reproduces bit for bit -- is NOT the gradient of the reference's forward):
      Q10 (W = view3x3 instead of its transpose) corrupts the covariance path: position, quaternion and log-scale;
      Q11 (+0.5 instead of -0.5 viewport.y) flips the y part of the position gradient that comes through the projected centre;
      Q23 (dL/dconic.y counted twice) corrupts everything that depends on the 2D covariance."""
    cfg, g, cam, st, gm, gc, go, gcol = _k17_case(orc, *_k17_scene(4))
    fd = _k17_fd(g, cam, gm, gc, go)
    got = _k17_oracle(orc, g, cam, st, gm, gc, go, gcol, flags=flags)
    for key in ("pos", "quat", "log_scale"):
        err = _rel(got[key], fd[key])
        if key in broken:
            assert err > 0.05, (key, err)
        else:
            assert err < 3e-3, (key, err)
    assert _rel(got["opacity_raw"], fd["opacity_raw"]) < 3e-3    # the opacity path has no deviation


# ----------------------------------------------------------------------------------------------------------------- (c) K18 Adam
def test_adam_is_the_closed_form_without_bias_correction(orc):
    """Three steps of the oracle's Adam (adam.wgsl:67-175) against Kingma & Ba's update in float64 WITHOUT bias correction,
    on all 14 trained scalars, with the quaternion renormalised after its update (adam.wgsl:113-130), Gaussians of a view that touched no
    tile left alone (Q15), position w forced to 1 and scale w to 0 (adam.wgsl:108, 142).  The bias-corrected textbook form is far away,
    so the test can tell the two apart."""
    rng = np.random.default_rng(7)
    n = 3000
    st = orc.new_optimizer_state(n)
    st["opt_pos"][:, 0:3] = rng.normal(0, 2, (n, 3)); st["opt_pos"][:, 3] = 1.0
    q = rng.normal(0, 1, (n, 4)); st["opt_rot"][:, 0:4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    st["opt_scale"][:, 0:3] = rng.uniform(-6, -2, (n, 3))
    st["opt_opacity"][:, 0] = rng.normal(0, 1, n)
    st["param_sh"][:] = rng.uniform(-1, 1, (n, 48))
    for k in ("opt_pos", "opt_rot", "opt_scale"):
        st[k][:, 4:8] = rng.normal(0, 1e-3, (n, 4)); st[k][:, 8:12] = rng.uniform(0, 1e-5, (n, 4))
    for k in ("opt_pos", "opt_scale"):     # the fourth lane of the two vec3 groups carries no moments (adam.wgsl:108, 142)
        st[k][:, [7, 11]] = 0.0
    st["opt_opacity"][:, 1] = rng.normal(0, 1e-3, n); st["opt_opacity"][:, 2] = rng.uniform(0, 1e-5, n)
    st["state_sh"][:, 0:6] = np.stack([rng.normal(0, 1e-3, (n, 3)), rng.uniform(0, 1e-5, (n, 3))], 2).reshape(n, 6)
    st = {k: v.astype(np.float32) for k, v in st.items()}
    ref = {k: v.astype(np.float64) for k, v in st.items()}
    corrected = {k: v.copy() for k, v in ref.items()}
    cfg = orc.ADAM_DEFAULT.copy()
    lr = dict(pos=float(cfg[0]), color=float(cfg[1]), opacity=float(cfg[2]), scale=float(cfg[3]), rot=float(cfg[4]))
    b1, b2, eps = float(cfg[5]), float(cfg[6]), float(cfg[7])
    frozen_sh = st["param_sh"][:, 3:].copy()
    for step in range(1, 4):
        g16 = rng.normal(0, 1, (n, 16)).astype(np.float16)
        g16[:, [11, 15]] = 0
        grads = np.ascontiguousarray(g16).view(np.uint32).reshape(n, 8)
        counts = (rng.uniform(size=n) < 0.8).astype(np.uint32) * rng.integers(1, 9, n).astype(np.uint32)
        orc.adam(cfg, counts, grads, st)
        g = g16.astype(np.float64)
        vis = counts != 0
        for tgt, bias in ((ref, False), (corrected, True)):
            def upd(p, gr, m, v, rate):
                m2, v2 = b1 * m + (1 - b1) * gr, b2 * v + (1 - b2) * gr * gr
                mh, vh = (m2 / (1 - b1 ** step), v2 / (1 - b2 ** step)) if bias else (m2, v2)
                return p - rate * mh / (np.sqrt(vh) + eps), m2, v2
            for key, gcols, rate, width in (("opt_pos", slice(0, 3), lr["pos"], 3), ("opt_rot", slice(4, 8), lr["rot"], 4), ("opt_scale", slice(8, 11), lr["scale"], 3)):
                a = tgt[key]
                p, m, v = upd(a[vis, 0:width], g[vis, gcols], a[vis, 4:4 + width], a[vis, 8:8 + width], rate)
                if key == "opt_rot":
                    p = p / np.linalg.norm(p, axis=1, keepdims=True)
                a[vis, 0:width], a[vis, 4:4 + width], a[vis, 8:8 + width] = p, m, v
            o = tgt["opt_opacity"]
            o[vis, 0], o[vis, 1], o[vis, 2] = upd(o[vis, 0], g[vis, 3], o[vis, 1], o[vis, 2], lr["opacity"])
            s_ = tgt["state_sh"]
            for c in range(3):
                tgt["param_sh"][vis, c], s_[vis, 2 * c], s_[vis, 2 * c + 1] = upd(tgt["param_sh"][vis, c], g[vis, 12 + c], s_[vis, 2 * c], s_[vis, 2 * c + 1], lr["color"])

    def dist(a, b):
        return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    for k in st:
        assert dist(st[k].astype(np.float64), ref[k]) < 2e-6, (k, dist(st[k].astype(np.float64), ref[k]))
    assert dist(st["opt_pos"][:, 0:3].astype(np.float64), corrected["opt_pos"][:, 0:3]) > 1e-4   # bias correction would be a different optimizer
    assert np.allclose(np.linalg.norm(st["opt_rot"][:, 0:4], axis=1), 1.0, atol=2e-6)
    assert np.all(st["opt_pos"][:, 3] == 1.0) and np.all(st["opt_scale"][:, 3] == 0.0)
    assert np.array_equal(st["param_sh"][:, 3:], frozen_sh)       # only the DC coefficients are trained (Q14)


# ----------------------------------------------------------------------------------------------------------------- (d) K26-K30
def test_densify_decisions_capacity_and_children(orc):
    """K26-K30 restated from the rules (densify-prune-decide / -cap / -scatter-*.wgsl), vectorised in float64, against the oracle:
    actions, capped counts, offsets and total exactly; every child's position, log-scale and opacity within one fp16 ulp (working copy) or
    1e-6 (fp32 masters); state carry-over / reset and the always-zeroed opacity moments (Q16) exactly."""
    cfg = harness.small_config("c1", num_points=6000, s0=0.1)            # scales 0.1 .. 1: both clone and split occur
    g, sh = synth.make_gaussians(cfg)
    n = g.shape[0]
    rng = np.random.default_rng(11)
    metric = rng.integers(0, 12, n).astype(np.uint32)
    gs = ind.unpack_gaussians(g)
    clone_thr, prune_op, split_scale = 6, 0.15, 0.5
    max_out = n + 700                                                     # binds: the tail of the cloud is cut off by the capacity rule
    prep = orc.densify_prepare(g, metric, max_out, clone_threshold=clone_thr, prune_opacity=prune_op, split_scale=split_scale)

    sig = ind.sigmoid(gs["opacity_raw"])
    act = np.where(sig < prune_op, 3, np.where(metric >= clone_thr, np.where(np.exp(gs["log_scale"]).max(1) >= split_scale, 2, 1), 0))
    cnt = np.where(act == 3, 0, np.where(act == 0, 1, 2))
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    act = np.where(off >= max_out, 3, np.where((cnt == 2) & (off == max_out - 1), 0, act))     # cap rule (densify-prune-cap.wgsl:32-49)
    cnt = np.where(off >= max_out, 0, np.where((cnt == 2) & (off == max_out - 1), 1, cnt))
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    assert np.array_equal(prep["actions"], act) and np.array_equal(prep["counts"], cnt) and np.array_equal(prep["offsets"], off)
    assert prep["total"] == int(cnt.sum()) <= max_out and (act == 1).sum() > 50 and (act == 2).sum() > 50 and (act == 3).sum() > 50
    assert (off >= 0).all() and cnt[np.flatnonzero(np.cumsum(cnt) > max_out)].sum() == 0

    st = orc.unpack(g, sh)
    for k in ("opt_pos", "opt_rot", "opt_scale"):
        st[k][:, 4:] = rng.uniform(0.1, 1.0, (n, 8)).astype(np.float32)
    st["opt_opacity"][:, 1:] = rng.uniform(0.1, 1.0, (n, 2)).astype(np.float32)
    st["state_sh"][:] = rng.uniform(0.1, 1.0, (n, 96)).astype(np.float32)
    st["opt_pos"][:, 0:3] += rng.normal(0, 1e-3, (n, 3)).astype(np.float32)   # masters differ from the fp16 copy (Q17)
    out_n = prep["total"]
    og, osh, ost = orc.densify_scatter(g, sh, st, prep, out_n)

    src = np.repeat(np.arange(n), cnt)
    dst = np.arange(out_n)
    variant = dst - off[src]
    a = act[src]
    # ---- working copy (fp16): perturbed from the fp16 values
    want_pos, want_ls = _densify_children_fp64(gs["pos"][src], gs["quat"][src], gs["log_scale"][src], src, dst, a, variant)
    clamp = sig[src] > 0.8
    want_op = np.where(clamp, 1.38629436112, gs["opacity_raw"][src])
    got = ind.unpack_gaussians(og)
    moved = (a == 2) | ((a == 1) & (variant == 1))
    # (a child coordinate that lands near zero is the difference of two O(1) float32 numbers: there one fp16 ulp is below float32's
    # own rounding, and the absolute error is what counts)
    assert ((ind.f16_ulp_distance(ind.f16_bits(got["pos"]), ind.f16_bits(want_pos)) <= 1) | (np.abs(got["pos"] - want_pos) < 2e-6)).all()
    assert np.array_equal(got["pos"][~moved], gs["pos"][src][~moved])                               # verbatim where nothing moves
    assert ind.f16_ulp_distance(ind.f16_bits(got["log_scale"]), ind.f16_bits(want_ls)).max() <= 1
    assert np.array_equal(got["log_scale"][a != 2], gs["log_scale"][src][a != 2])
    assert np.array_equal(ind.f16_bits(got["opacity_raw"]), ind.f16_bits(want_op))
    assert np.array_equal(got["quat"], gs["quat"][src]) and np.array_equal(osh, sh[src])
    d = np.linalg.norm(got["pos"] - gs["pos"][src], axis=1)
    assert d[moved].min() > 0 and (d[(a == 2)] > 0).all()
    # ---- fp32 masters: the same perturbation from the MASTER position / rotation / scale; moments carried or reset
    m_pos, m_ls = _densify_children_fp64(st["opt_pos"][src, 0:3].astype(np.float64), st["opt_rot"][src, 0:4].astype(np.float64),
                                         st["opt_scale"][src, 0:3].astype(np.float64), src, dst, a, variant)
    assert np.abs(ost["opt_pos"][:, 0:3] - m_pos).max() < 2e-6 * max(1.0, np.abs(m_pos).max())
    want_scale = st["opt_scale"][src, 0:3].astype(np.float64) - np.where(a == 2, 0.4700036292457356, 0.0)[:, None]
    assert np.abs(ost["opt_scale"][:, 0:3] - want_scale).max() < 2e-6
    assert np.array_equal(ost["opt_rot"][:, 0:4], st["opt_rot"][src, 0:4]) and np.array_equal(ost["param_sh"], st["param_sh"][src])
    new = (variant == 1) | (a == 2)
    for k in ("opt_pos", "opt_rot", "opt_scale"):
        assert np.all(ost[k][new, 4:] == 0) and np.array_equal(ost[k][~new, 4:], st[k][src][~new, 4:]), k
    assert np.all(ost["state_sh"][new] == 0) and np.array_equal(ost["state_sh"][~new], st["state_sh"][src][~new])
    assert np.all(ost["opt_opacity"][:, 1:] == 0)                                                       # Q16: opacity moments always zeroed
    m_sig = ind.sigmoid(st["opt_opacity"][src, 0].astype(np.float64))
    assert np.array_equal(ost["opt_opacity"][:, 0], np.where(m_sig > 0.8, np.float32(1.38629436112), st["opt_opacity"][src, 0]))


# ----------------------------------------------------------------------------------------------------------------- (e) K15
def _loss_gradient_fp64(pred_u8, targ_u8, l1, l2, ld, c1, c2):
    """loss.wgsl:25-115 from its formulas: L1 / L2 terms per channel plus the (non-differentiated-statistics) DSSIM term
    0.5 (1 - SSIM) (x - y) with 5x5 box statistics sampled clamp-to-edge; alpha lane 1."""
    from scipy.ndimage import uniform_filter
    x, y = pred_u8[..., :3].astype(np.float64) / 255.0, targ_u8[..., :3].astype(np.float64) / 255.0
    box = lambda a: uniform_filter(a, size=(5, 5, 1), mode="nearest")
    mx, my = box(x), box(y)
    sxx, syy, sxy = box(x * x) - mx * mx, box(y * y) - my * my, box(x * y) - mx * my     # == mean of centred products
    ssim = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    d = x - y
    out = np.ones(pred_u8.shape[:2] + (4,))
    out[..., :3] = l1 * np.sign(d) + l2 * d + (ld * 0.5 * (1 - ssim) * d if ld > 0 else 0.0)
    return out, ssim


@pytest.mark.parametrize("lam", [(0.8, 0.0, 0.2), (0.5, 0.3, 0.2), (1.0, 0.0, 0.0)], ids=["default", "with-l2", "l1-only"])
def test_k15_loss_gradient_is_the_formula(orc, lam):
    """K15 against a float64 restatement that uses scipy's box filter with edge replication (E[ab] - E[a]E[b] form; the shader sums
    centred products): every lane within 2e-6 on images with smooth and noisy regions, equal and unequal pixels, non-multiple-of-16
    size; and the DSSIM factor really is 0.5 (1 - SSIM) with SSIM in [-1, 1]."""
    rng = np.random.default_rng(5)
    h, w = 45, 71
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(xx / 9.0)[..., None] * np.cos(yy / 7.0)[..., None] * np.array([1.0, 0.7, -0.5, 0.0])
    pred = np.clip(base + rng.normal(0, 25, (h, w, 4)), 0, 255).astype(np.uint8)
    targ = np.clip(base + rng.normal(0, 6, (h, w, 4)), 0, 255).astype(np.uint8)
    targ[10:20, 10:30] = pred[10:20, 10:30]                      # an exactly matching region: sign(0) = 0, gradient 0
    pred[30:, :8] = 0; targ[30:, :8] = 255                       # saturated difference at an image edge
    cfg = orc.training_config(lambda_l1=lam[0], lambda_l2=lam[1], lambda_dssim=lam[2])
    got = orc.loss_grad(pred, targ, cfg)
    want, ssim = _loss_gradient_fp64(pred, targ, float(cfg[0]), float(cfg[1]), float(cfg[2]), float(cfg[3]), float(cfg[4]))
    assert got.shape == want.shape and np.all(got[..., 3] == 1.0)
    assert np.abs(got - want).max() < 2e-6, np.abs(got - want).max()
    assert np.all(got[10:20, 10:30, :3] == 0)
    assert ssim.min() >= -1 - 1e-9 and ssim.max() <= 1 + 1e-9 and ssim[12:18, 12:28].min() > 0.999999      # identical windows: SSIM = 1
    assert np.abs(got[..., :3]).max() <= lam[0] + lam[1] + lam[2] + 1e-6


@pytest.mark.parametrize("lam", [(0.8, 0.0, 0.2), (0.5, 0.3, 0.2), (0.0, 0.0, 1.0)], ids=["default", "with-l2", "dssim-only"])
@pytest.mark.parametrize("w,h", [(7, 5), (65, 43)])
@pytest.mark.parametrize("kind", ["noise", "anti", "saturated"])
def test_k15_loss_gradient_is_the_formula_on_crafted_pairs(orc, kind, w, h, lam):
    """The same comparison, same 2e-6, on the crafted pairs the GPU kernel is compared with the oracle on (tests/lossimages.py): uncorrelated noise,
    windows of negative covariance (SSIM near -1, the factor 0.5 (1 - SSIM) near 1) and saturated differences that reach the image's edges, at a
    size smaller than two windows and at one that is no multiple of anything."""
    import lossimages
    pred, targ = lossimages.pair(kind, w, h, seed=w * 7919 + h * 31)
    cfg = orc.training_config(lambda_l1=lam[0], lambda_l2=lam[1], lambda_dssim=lam[2])
    got = orc.loss_grad(pred, targ, cfg)
    want, ssim = _loss_gradient_fp64(pred, targ, float(cfg[0]), float(cfg[1]), float(cfg[2]), float(cfg[3]), float(cfg[4]))
    worst = float(np.abs(got - want).max())
    print(f"K15 {kind} {w}x{h} {lam}: max |oracle - f64| = {worst:.3e}, SSIM in [{ssim.min():.6f}, {ssim.max():.6f}]")
    assert got.shape == want.shape and np.all(got[..., 3] == 1.0)
    assert worst < 2e-6, worst
    same = pred[..., :3] == targ[..., :3]
    assert np.all(got[..., :3][same] == 0)                        # sign(0) = 0, and every other term has the factor d = 0
    assert ssim.min() >= -1 - 1e-9 and ssim.max() <= 1 + 1e-9
    assert np.abs(got[..., :3]).max() <= lam[0] + lam[1] + lam[2] + 1e-6
    if kind == "anti":
        assert ssim.min() < -0.9, ssim.min()                     # the case is there for the negative branch: it must reach it
    if kind == "saturated":
        assert same[:, :2].all() and (w <= 2 or not same[:, 2:].any())


# ----------------------------------------------------------------------------------------------------------------- (f) K21-K24, K31
def test_k21_k23_metric_map_in_exact_integer_arithmetic(orc):
    """The per-pixel error is floor(1e6 * sum|d rgb| / 765) -- evaluated here in exact integers -- to within the one unit a float32
    product can fall short of an integer; min / max are those of the stored errors; the flag is (e - min) / (max - min) > threshold, exact
    except within 1e-6 of the threshold.  Constant images (max == min) flag nothing."""
    rng = np.random.default_rng(9)
    h, w = 37, 53
    pred = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    targ = np.clip(pred.astype(np.int64) + rng.integers(-40, 41, (h, w, 4)), 0, 255).astype(np.uint8)
    targ[0, 0] = pred[0, 0]                                       # a zero-error pixel
    for thr in (0.1, 0.5, 0.9):
        err, mm, flags = orc.metric_map(pred, targ, thr)
        s = np.abs(pred[..., :3].astype(np.int64) - targ[..., :3].astype(np.int64)).sum(-1)
        want = (s * 1_000_000) // 765
        assert np.abs(err.astype(np.int64) - want).max() <= 1 and (err.astype(np.int64) == want).mean() > 0.9
        assert mm[0] == err.min() == 0 and mm[1] == err.max()
        num, den = err.astype(np.int64) - int(mm[0]), int(mm[1]) - int(mm[0])
        exact = num > thr * den
        near = np.abs(num / den - thr) < 1e-6
        assert np.array_equal(flags.astype(bool)[~near], exact[~near]) and 0 < flags.sum() < flags.size
    err, mm, flags = orc.metric_map(pred, pred, 0.0)
    assert not err.any() and not flags.any() and mm[0] == mm[1] == 0


@pytest.mark.parametrize("shape", [((64, 96), (32, 48)), ((45, 71), (22, 35)), ((40, 40), (40, 40)), ((30, 50), (10, 25))],
                         ids=["half", "odd-half", "same-size", "third-by-half"])
def test_k31_downsample_is_the_linear_sampler(orc, shape):
    """The ground truth is drawn into the metric target with a linear sampler, clamp-to-edge (trainer.ts:303-328): float64 restatement
    of bilinear sampling at destination texel centres, then unorm8 rounding; the oracle may differ by one level only where the float64
    value sits within 1e-4 of a rounding boundary.  Exact halving is the 2x2 box average; same size is the identity."""
    (sh_, sw_), (dh, dw) = shape
    rng = np.random.default_rng(13)
    src = rng.integers(0, 256, (sh_, sw_, 4), dtype=np.uint8)
    got = orc.downsample_bilinear(src, dw, dh)
    u = (np.arange(dw) + 0.5) / dw * sw_ - 0.5
    v = (np.arange(dh) + 0.5) / dh * sh_ - 0.5
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    wu, wv = (u - x0)[None, :, None], (v - y0)[:, None, None]
    cx = lambda a: np.clip(a, 0, sw_ - 1)
    cy = lambda a: np.clip(a, 0, sh_ - 1)
    s = src.astype(np.float64)
    top = s[cy(y0)][:, cx(x0)] * (1 - wu) + s[cy(y0)][:, cx(x0 + 1)] * wu
    bot = s[cy(y0 + 1)][:, cx(x0)] * (1 - wu) + s[cy(y0 + 1)][:, cx(x0 + 1)] * wu
    val = top * (1 - wv) + bot * wv
    want = np.floor(val + 0.5)
    on_boundary = np.abs(val + 0.5 - np.round(val + 0.5)) < 1e-4
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert diff[~on_boundary].max() == 0 and diff.max() <= 1
    if (sh_, sw_) == (2 * dh, 2 * dw):
        box = s.reshape(dh, 2, dw, 2, 4).mean((1, 3))
        assert np.abs(val - box).max() < 1e-9
    if (sh_, sw_) == (dh, dw):
        assert np.array_equal(got, src)


def test_k24_metric_counts_are_the_flagged_contributions(orc):
    """K24 recounted in float64 from the forward pass's own lists: for every flagged pixel, +1 for each of the first n_contrib entries of
    its tile whose alpha = min(0.99, sigma * exp(-q/2)) reaches 1/255 (no extent test: SURVEY Q21).  Identical except where the float64
    alpha is within 1e-4 (relative) of the cut."""
    cfg, g, sh, cam = _scene(base="c1", n=3000, w=96, h=64, view=2)
    st, ti = synth.render_settings(cfg), synth.tile_info(cfg.width, cfg.height, 0)
    fw = orc.forward(g, sh, cam, st, ti)
    rng = np.random.default_rng(3)
    flags = (rng.random((cfg.height, cfg.width)) < 0.3).astype(np.uint32)
    n = g.shape[0]
    counts = np.zeros(n, np.uint32)
    e = fw["total_entries"]
    orc.metric_count(st, fw["tile_ranges"], fw["sorted_values"][:e].copy(), e, fw["splats"], flags, fw["n_contrib"], counts)

    sp = fw["splats"].view(np.float16).reshape(-1, 12).astype(np.float64)
    centre = (sp[:, 0:2] * np.array([0.5, -0.5]) + 0.5) * np.array([cfg.width, cfg.height])
    want = np.zeros(n, np.int64)
    unsure = np.zeros(n, bool)
    ntx = (cfg.width + 15) // 16
    nc = fw["n_contrib"].reshape(cfg.height, cfg.width)
    for py, px in zip(*np.nonzero(flags)):
        k = int(nc[py, px])
        start = int(fw["tile_ranges"][(py // 16) * ntx + px // 16])
        if k == 0 or start == 0xFFFFFFFF:
            continue
        ids = fw["sorted_values"][start:start + k].astype(np.int64)
        d = np.array([px + 0.5, py + 0.5]) - centre[ids]
        q = sp[ids, 4] * d[:, 0] ** 2 + 2 * sp[ids, 5] * d[:, 0] * d[:, 1] + sp[ids, 6] * d[:, 1] ** 2
        alpha = np.minimum(0.99, sp[ids, 11] * np.exp(-0.5 * q))
        np.add.at(want, ids, alpha >= 1 / 255)
        np.logical_or.at(unsure, ids, np.abs(alpha * 255 - 1) < 1e-4)
    assert want.sum() > 1000
    assert np.array_equal(counts[~unsure], want[~unsure]) and np.abs(counts.astype(np.int64) - want).max() <= 1
