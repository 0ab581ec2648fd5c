"""CPU: the oracle's Adam, re-pack and gradient unpack on the crafted inputs of tests/adamcases.py -- against the float64 closed form with a
lane-by-lane rounding bound, and class by class (which lanes go non-finite, what a zero count leaves alone, that the padding halves are never
read, that subnormal moments are kept, what the re-pack saturates).  tests/test_gpu_optimizer_kernels.py compares the kernels with the oracle
on the same inputs bit for bit; this file is what keeps that comparison from agreeing with a wrong reference, or from passing on inputs that
do not contain what they are meant to."""
import numpy as np
import pytest

import adamcases as ac
import indep64

U = 2.0 ** -24          # unit roundoff of f32
BOUND = 16.0            # 12 correctly rounded f32 operations on the parameter path (3 for m', 4 for v', sqrt, + eps, lr *, /, +), room for second order
TINY = 2.0 ** -126      # smallest normal f32
KEYS = tuple(ac.STATE_WIDTHS)


def _normal(x):
    """Zero, or finite and at least the smallest normal f32 in magnitude."""
    a = np.abs(x)
    return np.isfinite(x) & ((a == 0) | ((a >= TINY) & (a < 2.0 ** 128)))


def _closed_form(st, g, h):
    """float64 Adam without bias correction on the 14 trained scalars, fed the f32-rounded hyperparameters.  Returns p', m', v', the two magnitude
    scales M_m and M_p of the bounds, and the mask of lanes on which every operand and every intermediate is zero or a normal f32."""
    p, m, v = (a.astype(np.float64) for a in ac.trained_pmv(st))
    with np.errstate(invalid="ignore"):
        g = g.astype(np.float64)
    b1, b2, eps = float(h[5]), float(h[6]), float(h[7])
    lr = np.array([float(h[t[6]]) for t in ac.TRAINED])[None, :]
    with np.errstate(all="ignore"):
        p2, m2, v2 = indep64.adam_update(p, g, m, v, lr, b1, b2, eps)
        mm = np.abs(b1 * m) + np.abs((1 - b1) * g)
        den = np.sqrt(v2) + eps
        mp = np.abs(p) + lr * mm / den
        ok = np.ones(p.shape, bool)
        for x in (p, m, v, g, b1 * m, (1 - b1) * g, b2 * v, (1 - b2) * g, (1 - b2) * g * g, m2, v2, lr * m2, np.sqrt(v2), den, lr * m2 / den, p2):
            ok &= _normal(x)
    return p2, m2, v2, mm, mp, ok


def _units(got, want, scale):
    """|got - want| in units of 2^-24 * scale; where the scale is 0 the two must be equal."""
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - want)
        return np.where(scale > 0, d / (U * scale), np.where(d == 0, 0.0, np.inf))


def _worst_units(orc, case, h, form):
    st = ac.copy_state(case.state)
    if form == "packed":
        g = ac.used_f32(case.packed)
        orc.adam(h, case.counts, case.packed, st)
    else:
        g = case.grad32
        orc.adam_f32(h, case.counts, case.grad32, st)
    p2, m2, v2, mm, mp, ok = _closed_form(case.state, g, h)
    po, mo, vo = ac.trained_pmv(st)
    upd = (case.counts != 0)[:, None] & ok
    rot = list(ac.ROT_LANES)
    plain = upd.copy()
    plain[:, rot] = False
    em, ev, ep = _units(mo, m2, mm), _units(vo, v2, v2), _units(po, p2, mp)
    # the quaternion: both sides re-normalised in float64, the bound's scale divided by the float64 norm
    with np.errstate(all="ignore"):
        q2, qo = p2[:, rot], po[:, rot].astype(np.float64)
        n2, no = np.sqrt((q2 * q2).sum(1, keepdims=True)), np.sqrt((qo * qo).sum(1, keepdims=True))
        qok = upd[:, rot].all(1, keepdims=True) & _normal(n2 * n2) & (n2 > 0) & np.isfinite(qo).all(1, keepdims=True) & (no > 0)
        eq = _units(qo / no, q2 / n2, mp[:, rot] / n2)
    worst = dict(m=float(np.max(np.where(upd, em, 0), initial=0)), v=float(np.max(np.where(upd, ev, 0), initial=0)),
                 p=float(np.max(np.where(plain, ep, 0), initial=0)), q=float(np.max(np.where(qok, eq, 0), initial=0)))
    checked = int(upd.sum())
    return worst, checked, upd, (case.counts != 0)


@pytest.mark.parametrize("form", ["packed", "f32"])
@pytest.mark.parametrize("kind", ac.KINDS)
def test_the_oracle_is_within_rounding_of_the_float64_closed_form(orc, kind, form):
    report = {}
    for name, h in ac.HYPER.items():
        for n in ac.ONE_STEP_SIZES:
            case = ac.build(kind, n, hyper=h)
            worst, checked, upd, visible = _worst_units(orc, case, h, form)
            if kind in ("lanes", "magnitudes", "padding", "counts"):     # every lane of these is finite and normal: none may drop out of the check
                assert np.array_equal(upd, np.broadcast_to(visible[:, None], upd.shape)), f"{kind} {name} n={n}: lanes left the normal range"
                assert checked >= 12 * int(visible.sum()), f"{kind} {name} n={n}: only {checked} lanes are checked"
            # (of the other kinds, whichever lanes stay finite and normal: the parameters of `saturating`, the untouched lanes of `nonfinite`, ...)
            for k, w in worst.items():
                report[k] = max(report.get(k, 0.0), w)
                assert w <= BOUND, f"{kind} {form} {name} n={n}: {k} is {w:.2f} units of 2^-24 M from the float64 form (bound {BOUND})"
    print(f"{kind} {form}: worst rounding error in units of 2^-24 M: " + ", ".join(f"{k} {w:.2f}" for k, w in report.items()))
    assert max(report.values()) <= BOUND, f"{kind} {form}: worst {report}"


def _run(orc, case, h, form="packed", packed=None):
    st = ac.copy_state(case.state)
    if form == "packed":
        orc.adam(h, case.counts, case.packed if packed is None else packed, st)
    else:
        orc.adam_f32(h, case.counts, case.grad32, st)
    return st


@pytest.mark.parametrize("form", ["packed", "f32"])
def test_nonfinite_gradients_reach_exactly_the_predicted_lanes(orc, form):
    for name, h in ac.HYPER.items():
        for n in ac.ONE_STEP_SIZES:
            case = ac.build("nonfinite", n)
            st = _run(orc, case, h, form)
            pred = ac.nonfinite_prediction(n, case.counts)
            for k in KEYS:
                assert np.all(np.isfinite(case.state[k]))
                assert np.array_equal(~np.isfinite(st[k]), pred[k]), f"{form} {name} n={n}: non-finite entries of {k} are not the predicted ones"
    lane, which = ac.nonfinite_lane(ac.N_DEFAULT)
    assert set(lane.tolist()) == set(range(-1, 14)) and {(l, w) for l, w in zip(lane.tolist(), which.tolist()) if l >= 0} == {(l, w) for l in range(14) for w in range(5)}


@pytest.mark.parametrize("form", ["packed", "f32"])
def test_a_zero_count_leaves_the_gaussian_alone_and_only_zero_does(orc, form):
    for name, h in ac.HYPER.items():
        case = ac.build("counts", ac.N_DEFAULT)
        st = _run(orc, case, h, form)
        one = _run(orc, case._replace(counts=(case.counts != 0).astype(np.uint32)), h, form)
        zero = case.counts == 0
        assert set(case.counts.tolist()) == set(ac.COUNT_VALUES.tolist())
        for k in KEYS:
            assert np.array_equal(st[k][zero].view(np.uint32), case.state[k][zero].view(np.uint32)), f"{form} {name}: {k} changed under a zero count"
            assert np.array_equal(st[k].view(np.uint32), one[k].view(np.uint32)), f"{form} {name}: {k} depends on the count's value"
        p0, m0, v0 = ac.trained_pmv(case.state)
        p1, m1, v1 = ac.trained_pmv(st)
        assert np.all((m1 != m0)[~zero]) and np.all((v1 != v0)[~zero]), "every lane of an updated Gaussian moves"


def test_the_padding_halves_are_never_read(orc):
    for name, h in ac.HYPER.items():
        case = ac.build("padding", ac.N_DEFAULT)
        pad = ac.halves_of(case.packed)[:, ac.PAD_HALVES]
        assert np.all((pad != 0).any(1)) and np.isnan(pad.view(np.float16)).any() and np.isinf(pad.view(np.float16)).any()
        a, b = _run(orc, case, h), _run(orc, case, h, packed=ac.zero_padding(case.packed))
        for k in KEYS:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{name}: {k} depends on the padding halves"
            assert np.all(np.isfinite(a[k]))
    assert np.array_equal(ac.used_f32(case.packed), ac.used_f32(ac.zero_padding(case.packed)))


@pytest.mark.parametrize("form", ["packed", "f32"])
def test_decayed_moments_stay_subnormal(orc, form):
    """The oracle keeps subnormal moments (no flush to zero), and the inputs do reach that range: more than a quarter of the updated Gaussians come
    out with a subnormal m' or v' under every hyperparameter set."""
    def subnormal(x):
        a = np.abs(x)
        return (a > 0) & (a < np.float32(TINY))
    for name, h in ac.HYPER.items():
        case = ac.build("decayed", ac.N_DEFAULT)
        st = _run(orc, case, h, form)
        _, m1, v1 = ac.trained_pmv(st)
        upd = case.counts != 0
        hit = (subnormal(m1) | subnormal(v1)).any(1) & upd
        share = hit.sum() / upd.sum()
        print(f"decayed {form} {name}: {share:.2f} of the updated Gaussians have a subnormal m' or v'")
        assert share > 0.25, f"{form} {name}: only {share:.2f}"
        # and they are what float64 gives, rounded once to the f32 grid (spacing 2^-149 down there)
        g = ac.used_f32(case.packed) if form == "packed" else case.grad32
        _, m2, v2, _, _, _ = _closed_form(case.state, g, h)
        sm, sv = subnormal(m1) & upd[:, None], subnormal(v1) & upd[:, None]
        assert np.all(np.abs(m1.astype(np.float64) - m2)[sm] <= 2.0 ** -149 * 2), f"{form} {name}: a subnormal m' is off the float64 value"
        assert np.all(np.abs(v1.astype(np.float64) - v2)[sv] <= 2.0 ** -149 * 2), f"{form} {name}: a subnormal v' is off the float64 value"
    if form == "f32":
        h = ac.HYPER["default"]
        g = case.grad32.astype(np.float64)
        t = (1 - float(h[6])) * g * g
        assert np.any((t > 0) & (t < TINY)), "no fp32 sum makes (1 - beta2) g^2 subnormal"


def test_repack_saturates_where_predicted(orc):
    def h16(x):     # numpy's own f32 -> f16: nearest even, overflow to inf
        with np.errstate(over="ignore"):
            return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)

    for name, h in ac.HYPER.items():
        for n in ac.ONE_STEP_SIZES:
            case = ac.build("saturating", n, hyper=h)
            st = _run(orc, case, h)
            g, sh = np.zeros((n, 6), np.uint32), ac.sh_rows(n)
            before = sh.copy()
            orc.repack(st, g, sh)
            got = ac.trained_halves(g, sh)
            p0, _, _ = ac.trained_pmv(case.state)
            p1, _, _ = ac.trained_pmv(st)
            other = [l for l in range(14) if l not in ac.ROT_LANES]
            assert np.array_equal(p1[:, other].view(np.uint32), p0[:, other].view(np.uint32)), f"{name} n={n}: a crafted parameter moved"
            want = h16(p0)
            assert np.array_equal(got[:, other], want[:, other]), f"{name} n={n}: re-packed halves"
            rot = got[:, list(ac.ROT_LANES)]
            kind = ac.saturating_rot_kind(n)
            isnan = ((rot & 0x7C00) == 0x7C00) & ((rot & 0x03FF) != 0)
            assert np.all(isnan[(kind == 1) | (kind == 2)]), f"{name} n={n}: a zero quaternion must re-pack as four NaN halves"
            assert np.all(st["opt_rot"][kind == 1, 0:4] != st["opt_rot"][kind == 1, 0:4]), f"{name} n={n}: the update did not land on exactly zero"
            assert np.all((rot[kind == 3] & 0x7FFF) == 0), f"{name} n={n}: a quaternion whose squared norm overflows normalises to zero"
            assert np.array_equal(rot[kind == 0], h16(np.array([0.5, -0.5, 0.5, 0.5]))[None, :].repeat(int((kind == 0).sum()), 0))
            assert np.array_equal(g[:, 5] >> 16, np.zeros(n, np.uint32))
            # the rest of the SH row: the oracle passes word 1's high half through f16 -> f32 -> f16, which may only change a NaN's payload
            hb, ha = before.view(np.uint16).reshape(n, 48), sh.view(np.uint16).reshape(n, 48)
            nan3 = ((hb[:, 3] & 0x7C00) == 0x7C00) & ((hb[:, 3] & 0x03FF) != 0)
            assert np.array_equal(ha[:, 4:], hb[:, 4:]) and np.array_equal(ha[~nan3, 3], hb[~nan3, 3])
    want = h16(ac.SATURATING_VALUES)
    assert 0x7C00 in want and 0xFC00 in want and 0x8000 in want and 0x7BFF in want and 0xFBFF in want and 0x7BFE in want
    assert np.any((want & 0x7C00 == 0) & (want & 0x3FF != 0)), "no fp16 subnormal among the crafted values"


def test_gradient_views_hold_the_three_special_sums(orc):
    for n in ac.ONE_STEP_SIZES[1:]:
        views = ac.gradient_views(n)
        unpacked = [orc.unpack_gradients_f32(p) for p, _ in views]
        for (p, _), u in zip(views, unpacked):
            assert np.array_equal(u.view(np.uint32), ac.used_f32(p).view(np.uint32)) and np.array_equal(u.view(np.uint32), ac.used_f32(ac.zero_padding(p)).view(np.uint32))
            pad = ac.halves_of(p)[:, ac.PAD_HALVES]
            assert np.all((pad != 0).any(1))
        counts = [c for _, c in views]
        sums, visible = ac.gradient_sums(unpacked, counts)
        vis = [c != 0 for c in counts]
        assert np.array_equal(visible, sum(v.astype(np.uint32) for v in vis)) and set(visible.tolist()) == {0, 1, 2, 3}
        u0, u1 = unpacked[0], unpacked[1]
        both = (vis[0] & vis[1])[:, None]
        assert np.any(both & np.isinf(u0) & np.isinf(u1) & (u0 == -u1) & np.isnan(sums)), "no inf + (-inf) lane"
        only01 = (vis[0] & vis[1] & ~vis[2])[:, None]
        neg0 = (u0 == 0) & np.signbit(u0)
        assert np.any(only01 & neg0 & (u1 == 0) & ~np.signbit(u1) & (sums == 0) & ~np.signbit(sums)), "no (-0) + (+0) lane"
        assert np.any(only01 & (u0 != 0) & np.isfinite(u0) & (u1 == -u0) & (sums == 0)), "no cancellation to exactly zero"
        # a zero count: the first view stores +0, a later one adds nothing
        assert np.any(~vis[0]) and np.any(~vis[0] & ~vis[1] & ~vis[2]) and np.all(sums[visible == 0].view(np.uint32) == 0)
        # the sums round: float64 addition of the same values differs somewhere
        with np.errstate(invalid="ignore"):
            exact = sum(np.where(v[:, None], u.astype(np.float64), 0.0) for v, u in zip(vis, unpacked))
            assert np.any(np.isfinite(exact) & (exact != sums))


def test_the_builders_are_deterministic_and_distinct():
    a, b = ac.build("magnitudes", 257), ac.build("magnitudes", 257)
    for k in KEYS:
        assert np.array_equal(a.state[k].view(np.uint32), b.state[k].view(np.uint32))
    st = ac.lanes_state(ac.N_DEFAULT, fourth_lanes=True)
    allv = np.concatenate([np.abs(st[k]) for k in KEYS], axis=1)
    assert np.unique(allv).size == allv.size, "two state lanes of `lanes` hold the same magnitude"
    assert all(np.all(st[k][:, c] > 0) for k, w in ac.STATE_WIDTHS.items() for c in range(w) if ac.is_second_moment(k, c))
    packed, g32 = ac.lanes_gradients(ac.N_DEFAULT)
    assert np.unique(np.abs(ac.used_f32(packed))).size == 14 * ac.N_DEFAULT and np.unique(np.abs(g32)).size == 14 * ac.N_DEFAULT
    g = ac.halves_of(ac.build("magnitudes", ac.N_DEFAULT).packed)[:, ac.USED_HALVES]
    assert {0x0001, 0x7BFF, 0xFBFF, 0x0000, 0x8000}.issubset(set(g.reshape(-1).tolist())) and not np.any((g & 0x7C00) == 0x7C00)
    rows = ac.sh_rows(ac.N_DEFAULT).view(np.uint16).reshape(-1, 48)
    assert all(np.unique(r).size == 48 for r in rows)
    assert np.array_equal(ac.in_window(1000, 900, 0xFFFFFFFF), np.arange(1000) >= 900) and not ac.in_window(1000, 0xFFFFFFF0, 0x20).any()
