"""Crafted optimizer state, gradients and visibility counts for the optimizer kernels (webdgs_amd/csrc/optimizer.hip, adam.h).  Plain numpy:
nothing here needs a GPU, the library or the oracle.

A case is (state, packed, grad32, counts) for n Gaussians:
  state    the six reference-layout arrays, shaped as oracle.new_optimizer_state shapes them (opt_pos / opt_rot / opt_scale f32[n,12] =
           {param, m, v : vec4}, opt_opacity f32[n,3], param_sh f32[n,48], state_sh f32[n,96] = 48 x (m, v))
  packed   the packed fp16 gradient block u32[n,8]: halves 0-2 position, 3 opacity, 4-7 rotation, 8-10 log-scale, 12-14 colour; 11 and 15 unused
  grad32   the fp32 gradient block f32[n,14], the 14 used halves in that order
  counts   u32[n]: the Gaussian is updated where its count is not zero
The 14 trained scalars of a Gaussian are numbered like the columns of grad32 ("lanes"); TRAINED says where each one's {param, m, v} live and
which learning rate it takes.  tests/test_adam_cases.py holds the oracle to the float64 form on these inputs, tests/test_gpu_optimizer_kernels.py
the kernels to the oracle.
"""
from collections import namedtuple

import numpy as np

N_DEFAULT = 1000          # four workgroups of 256, the last one partial; the compact copy's plane pitch (a multiple of 16) is 1008
ONE_STEP_SIZES = (1, 257, 1000)
STATE_WIDTHS = dict(opt_pos=12, opt_rot=12, opt_scale=12, opt_opacity=3, param_sh=48, state_sh=96)   # 183 floats per Gaussian
KINDS = ("lanes", "magnitudes", "decayed", "saturating", "nonfinite", "padding", "counts")
COUNT_VALUES = np.array([0, 1, 7, 0x80000000, 0xFFFFFFFF], np.uint32)
USED_HALVES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14)
PAD_HALVES = (11, 15)

Case = namedtuple("Case", "state packed grad32 counts")

# lane -> (param array, column, m array, column, v array, column, index of its learning rate in the hyperparameter vector)
TRAINED = ([("opt_pos", j, "opt_pos", 4 + j, "opt_pos", 8 + j, 0) for j in range(3)] + [("opt_opacity", 0, "opt_opacity", 1, "opt_opacity", 2, 2)]
           + [("opt_rot", j, "opt_rot", 4 + j, "opt_rot", 8 + j, 4) for j in range(4)] + [("opt_scale", j, "opt_scale", 4 + j, "opt_scale", 8 + j, 3) for j in range(3)]
           + [("param_sh", c, "state_sh", 2 * c, "state_sh", 2 * c + 1, 1) for c in range(3)])
ROT_LANES = (4, 5, 6, 7)

# {lr_pos, lr_color, lr_opacity, lr_scale, lr_rot, beta1, beta2, epsilon}: the order of oracle.ADAM_DEFAULT and of wdgs_adam_hyperparameters
_DEFAULT = (0.00016, 0.0025, 0.05, 0.005, 0.001, 0.9, 0.999, 1e-8)


def _hyper(**kw):
    names = ("lr_pos", "lr_color", "lr_opacity", "lr_scale", "lr_rot", "beta1", "beta2", "epsilon")
    return np.array([kw.get(k, d) for k, d in zip(names, _DEFAULT)], np.float32)


HYPER = {
    "default": _hyper(),
    "beta1=0": _hyper(beta1=0.0),
    "beta2=0": _hyper(beta2=0.0),
    "slow-betas": _hyper(beta1=0.99, beta2=0.9999),
    "eps=1e-15": _hyper(epsilon=1e-15),
    "eps=1e-3": _hyper(epsilon=1e-3),
    "distinct-lr": _hyper(lr_pos=1.0, lr_color=0.5, lr_opacity=0.25, lr_scale=0.125, lr_rot=0.0625),
}
HYPER_NAMES = ("lr_pos", "lr_color", "lr_opacity", "lr_scale", "lr_rot", "beta1", "beta2", "epsilon")


def hyper_dict(h):
    """The vector as the keyword form ops.Optimizer(params=...) takes; the values stay the f32 ones."""
    return {k: float(v) for k, v in zip(HYPER_NAMES, np.asarray(h, np.float32))}


def new_state(n):
    return {k: np.zeros((n, w), np.float32) for k, w in STATE_WIDTHS.items()}


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def _lane_offsets():
    off, out = 0, {}
    for k, w in STATE_WIDTHS.items():
        out[k] = off
        off += w
    return out


def is_second_moment(key, col):
    if key == "state_sh":
        return col % 2 == 1
    if key == "opt_opacity":
        return col == 2
    return key in ("opt_pos", "opt_rot", "opt_scale") and col >= 8


def constant_fourth_lanes(st):
    """Position w = 1, scale w = 0 and their moments 0: what the reference's Adam writes there, and what cs_flush hands back for every Gaussian."""
    st["opt_pos"][:, 3], st["opt_pos"][:, [7, 11]] = 1.0, 0.0
    st["opt_scale"][:, [3, 7, 11]] = 0.0
    return st


def lanes_state(n, fourth_lanes=False):
    """Each of the 183 floats of a Gaussian is 0.5 + lane/256 + idx/2^18 (exact in f32, no two equal for n <= 1024), first moments and the
    parameters of odd lanes negated, second moments positive and scaled by 2^-10.  fourth_lanes: leave the padding lanes of opt_pos / opt_scale
    filled as well (the documented deviation of cs_flush is pinned on those)."""
    st, offs = new_state(n), _lane_offsets()
    idx = np.arange(n, dtype=np.float64)[:, None]
    for k, w in STATE_WIDTHS.items():
        lane = offs[k] + np.arange(w, dtype=np.float64)[None, :]
        val = 0.5 + lane / 256.0 + idx / 2.0 ** 18
        second = np.array([is_second_moment(k, c) for c in range(w)])[None, :]
        sign = np.where(((offs[k] + np.arange(w)) % 2 == 1)[None, :] & ~second, -1.0, 1.0)
        st[k][:] = (np.where(second, val * 2.0 ** -10, val) * sign).astype(np.float32)
    return st if fourth_lanes else constant_fourth_lanes(st)


def pack_halves(h14, pad=None):
    """f16[n,14] (or u16 bit patterns) -> u32[n,8]; pad: u16[n,2] for halves 11 and 15 (zeros when None)."""
    h14 = np.asarray(h14)
    bits = h14.view(np.uint16) if h14.dtype == np.float16 else h14.astype(np.uint16)
    n = bits.shape[0]
    row = np.zeros((n, 16), np.uint16)
    row[:, USED_HALVES] = bits
    if pad is not None:
        row[:, PAD_HALVES] = pad
    return np.ascontiguousarray(row).view(np.uint32).reshape(n, 8)


def halves_of(packed):
    return np.ascontiguousarray(packed).view(np.uint16).reshape(-1, 16)


def zero_padding(packed):
    row = halves_of(packed).copy()
    row[:, PAD_HALVES] = 0
    return row.view(np.uint32).reshape(-1, 8)


def used_f32(packed):
    """The 14 used halves as f32[n,14] (exact)."""
    return np.ascontiguousarray(halves_of(packed).view(np.float16)[:, USED_HALVES].astype(np.float32))


def lanes_gradients(n):
    """fp16 bit patterns 0x2C00 + 14 idx + lane (2^-4 .. 856, all distinct), sign by (idx + lane) parity; the fp32 block is the same value times
    1 + (lane + 1) 2^-18, which no fp16 holds."""
    idx, lane = np.arange(n)[:, None], np.arange(14)[None, :]
    bits = (0x2C00 + 14 * idx + lane).astype(np.uint16) | np.where((idx + lane) % 2 == 1, 0x8000, 0).astype(np.uint16)
    packed = pack_halves(bits)
    g32 = (used_f32(packed).astype(np.float64) * (1.0 + (lane + 1) * 2.0 ** -18)).astype(np.float32)
    return packed, g32


def mixed_counts(n):
    """Every seventh Gaussian not visible, the others with the non-zero values of COUNT_VALUES in turn."""
    idx = np.arange(n)
    return np.where(idx % 7 == 3, 0, COUNT_VALUES[1 + idx % 4]).astype(np.uint32)


def _pow2(rng, shape, lo, hi, signed=True):
    """(+-) 2^U[lo, hi] with a random mantissa, as f32."""
    v = np.exp2(rng.uniform(lo, hi, shape))
    if signed:
        v = v * rng.choice([-1.0, 1.0], shape)
    return v.astype(np.float32)


def _fill_trained(st, p=None, m=None, v=None):
    """p, m, v: f32[n,14] per lane (None: leave)."""
    for lane, (pk, pc, mk, mc, vk, vc, _) in enumerate(TRAINED):
        if p is not None:
            st[pk][:, pc] = p[:, lane]
        if m is not None:
            st[mk][:, mc] = m[:, lane]
        if v is not None:
            st[vk][:, vc] = v[:, lane]
    return st


def trained_pmv(st):
    """(p, m, v) as f32[n,14] per lane."""
    n = st["opt_pos"].shape[0]
    p, m, v = (np.zeros((n, 14), np.float32) for _ in range(3))
    for lane, (pk, pc, mk, mc, vk, vc, _) in enumerate(TRAINED):
        p[:, lane], m[:, lane], v[:, lane] = st[pk][:, pc], st[mk][:, mc], st[vk][:, vc]
    return p, m, v


def random_finite_halves(rng, n):
    """fp16 bit patterns drawn uniformly from the finite ones: every binade, the subnormals and both zeros, both signs."""
    bits = rng.integers(0, 0x7C00, (n, 14)).astype(np.uint16) | (rng.integers(0, 2, (n, 14)).astype(np.uint16) << 15)
    edge = np.array([0x0001, 0x8001, 0x7BFF, 0xFBFF, 0x0000, 0x8000, 0x03FF, 0x0400, 0x83FF, 0x3C00], np.uint16)   # 2^-24, 65504, +-0, the subnormal edge, 1
    k = min(n, 40)
    bits[:k] = edge[(np.arange(k)[:, None] * 3 + np.arange(14)[None, :]) % edge.size]
    return bits


def _magnitudes(n, seed):
    rng = np.random.default_rng(1000 + seed)
    st = lanes_state(n)
    _fill_trained(st, p=_pow2(rng, (n, 14), -10, 10), m=_pow2(rng, (n, 14), -30, 16), v=_pow2(rng, (n, 14), -60, 32, signed=False))
    packed = pack_halves(random_finite_halves(rng, n))
    g32 = _pow2(rng, (n, 14), -24, 16)
    g32[rng.uniform(size=(n, 14)) < 0.05] = 0.0
    return Case(st, packed, g32, mixed_counts(n))


DECAYED_EXPONENTS = (-125, -126, -127, -128, -130, -133, -136, -140, -146, -149)


def _decayed(n):
    """m and v in and just above the f32 subnormal range (2^-126); zero gradients on the even Gaussians, the smallest fp16 subnormal on the odd
    ones; fp32 sums of 2^-60 .. 2^-72 there, whose (1 - beta2) g^2 is subnormal.  Half of the non-quaternion parameters are themselves tiny, so that
    a step computed from such moments is not lost in the addition."""
    st = lanes_state(n)
    idx, lane = np.arange(n)[:, None], np.arange(14)[None, :]
    e = np.array(DECAYED_EXPONENTS)
    mant = np.array([1.0, 1.5, 1.25, 1.75])
    m = np.ldexp(mant[(idx + lane) % 4], e[(idx + 3 * lane) % e.size]) * np.where((idx // 2 + lane) % 2 == 1, -1.0, 1.0)
    v = np.ldexp(mant[(idx + 2 * lane) % 4], e[(2 * idx + lane + 5) % e.size])
    p, _, _ = trained_pmv(st)
    tiny = ((idx + lane) % 2 == 1) & ~np.isin(lane, ROT_LANES)
    p = np.where(tiny, np.ldexp(p.astype(np.float64), -90 - ((idx + lane) % 31)), p)
    _fill_trained(st, p=p.astype(np.float32), m=m.astype(np.float32), v=v.astype(np.float32))
    odd = (idx % 2 == 1)
    bits = np.where(odd, np.where((idx // 2 + lane) % 2 == 1, 0x8001, 0x0001), 0).astype(np.uint16)
    g32 = np.where(odd, np.ldexp(mant[(idx + lane) % 4], -60 - ((idx // 2 + lane) % 13)) * np.where((idx // 2 + lane) % 2 == 1, -1.0, 1.0), 0.0).astype(np.float32)
    return Case(st, pack_halves(bits), g32, np.where(np.arange(n) % 11 == 10, 0, 1).astype(np.uint32))


_F16_MAX = 65504.0
# what leaves fp16 on re-pack, and what just does not: beyond +-65504; 65520 is the tie that rounds to inf and the f32 below it the last that gives
# 65504; 65488 is the tie between 65472 and 65504 (to even: 65472) and the f32 above it gives 65504; the fp16 subnormal range, its ties 2^-25 (to 0)
# and 1.5 * 2^-24 (to 2^-23), the f32 above 2^-25 (to 2^-24); f32 values far below; -0
SATURATING_VALUES = np.array(
    [70000.0, -70000.0, 3.0e38, -3.0e38, 65520.0, np.nextafter(np.float32(65520.0), np.float32(0)), -65520.0, 65488.0, np.nextafter(np.float32(65488.0), np.float32(1e9)),
     -65488.0, _F16_MAX, -_F16_MAX, 2.0 ** -14, 2.0 ** -15, -2.0 ** -15, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
     -2.0 ** -25, 1.5 * 2.0 ** -24, 3.0e-8, 2.0 ** -26, 1.0e-30, 2.0 ** -140, -0.0, 0.0, 0.75 * 2.0 ** -14, 1023.5 * 2.0 ** -24], np.float32)
SATURATING_ROT = ("ordinary", "lands-on-zero", "stays-zero", "overflows")


def saturating_rot_kind(n):
    return np.arange(n) % len(SATURATING_ROT)


def _saturating(n, hyper):
    """Zero gradients and zero moments nearly everywhere, so every parameter keeps its crafted value through the step and the re-pack sees exactly
    that value.  Quaternions by idx % 4: ordinary; (s, 0, 0, 0) with a first moment whose step is exactly -s under `hyper` (the f32 operations of
    adam_step on that one lane, in numpy); all zero; and one whose squared norm overflows f32 (the normalised quaternion is then all zero)."""
    h = np.asarray(hyper, np.float32)
    st = constant_fourth_lanes(new_state(n))
    idx, lane = np.arange(n)[:, None], np.arange(14)[None, :]
    p = SATURATING_VALUES[(idx * 5 + lane * 3) % SATURATING_VALUES.size]
    _fill_trained(st, p=p)
    kind = saturating_rot_kind(n)
    m0, v0 = np.float32(0.25), np.float32(0.0625)
    m1 = h[5] * m0 + (np.float32(1) - h[5]) * np.float32(0)
    v1 = h[6] * v0 + (np.float32(1) - h[6]) * np.float32(0) * np.float32(0)
    step = (-h[4] * m1) / (np.sqrt(v1) + h[7])
    rot = np.zeros((n, 12), np.float32)
    rot[kind == 0, 0:4] = np.array([0.5, -0.5, 0.5, 0.5], np.float32)
    rot[kind == 1, 0], rot[kind == 1, 4], rot[kind == 1, 8] = -step, m0, v0
    rot[kind == 3, 0:4] = np.array([2.0 ** 64, -2.0 ** 64, 0.0, 1.0], np.float32)
    st["opt_rot"][:] = rot
    full = lanes_state(n)     # the untrained SH coefficients and their moments: distinct, as in `lanes`
    st["param_sh"][:, 3:], st["state_sh"][:, 6:] = full["param_sh"][:, 3:], full["state_sh"][:, 6:]
    return Case(st, np.zeros((n, 8), np.uint32), np.zeros((n, 14), np.float32), np.ones(n, np.uint32))


NONFINITE_HALVES = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01], np.uint16)   # +inf, -inf, quiet NaN, a negative NaN with a payload, a signalling NaN
NONFINITE_F32 = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)


def nonfinite_lane(n):
    """The one lane of each Gaussian whose gradient is not finite (-1: none), and which of the five values it gets."""
    idx = np.arange(n)
    return np.where(idx % 15 == 14, -1, idx % 15), (idx // 15) % NONFINITE_HALVES.size


def _nonfinite(n):
    st = lanes_state(n)
    packed, g32 = lanes_gradients(n)
    lane, which = nonfinite_lane(n)
    row = halves_of(packed).copy()
    hit = np.flatnonzero(lane >= 0)
    row[hit, np.array(USED_HALVES)[lane[hit]]] = NONFINITE_HALVES[which[hit]]
    g32[hit, lane[hit]] = NONFINITE_F32[which[hit]]
    return Case(st, row.view(np.uint32).reshape(n, 8), g32, np.ones(n, np.uint32))


def nonfinite_prediction(n, counts=None):
    """bool masks shaped like the state: the entries that a non-finite gradient lane must make non-finite -- {param, m, v} of that scalar, and all four
    quaternion components when it is a rotation lane (they are normalised together) -- and no others."""
    lane, _ = nonfinite_lane(n)
    pred = {k: np.zeros((n, w), bool) for k, w in STATE_WIDTHS.items()}
    upd = np.ones(n, bool) if counts is None else (np.asarray(counts) != 0)
    for i in np.flatnonzero((lane >= 0) & upd):
        pk, pc, mk, mc, vk, vc, _ = TRAINED[lane[i]]
        pred[pk][i, pc] = pred[mk][i, mc] = pred[vk][i, vc] = True
        if lane[i] in ROT_LANES:
            pred["opt_rot"][i, 0:4] = True
    return pred


PAD_GARBAGE = np.array([0x7E00, 0x7C00, 0xFC00, 0xFFFF, 0x7BFF, 0x0001, 0xFBFF, 0x7C01, 0x3C00, 0xBEEF], np.uint16)


def garbage_padding(packed, shift=0):
    """Fills halves 11 and 15 with NaN, +-inf, +-65504 and other patterns; never both zero."""
    row = halves_of(packed).copy()
    idx = np.arange(row.shape[0])
    row[:, 11] = PAD_GARBAGE[(idx + shift) % PAD_GARBAGE.size]
    row[:, 15] = PAD_GARBAGE[(idx * 3 + 1 + shift) % PAD_GARBAGE.size]
    return row.view(np.uint32).reshape(-1, 8)


def _padding(n):
    c = _magnitudes(n, seed=5)
    return Case(c.state, garbage_padding(c.packed), c.grad32, c.counts)


def _counts(n):
    packed, g32 = lanes_gradients(n)
    return Case(lanes_state(n), packed, g32, COUNT_VALUES[np.arange(n) % COUNT_VALUES.size].copy())


def build(kind, n=N_DEFAULT, hyper=None, seed=0):
    """The case of that kind for n Gaussians.  Only `saturating` looks at `hyper` (its quaternion that lands on zero)."""
    if kind == "lanes":
        packed, g32 = lanes_gradients(n)
        return Case(lanes_state(n), packed, g32, mixed_counts(n))
    if kind == "magnitudes":
        return _magnitudes(n, seed)
    if kind == "decayed":
        return _decayed(n)
    if kind == "saturating":
        return _saturating(n, HYPER["default"] if hyper is None else hyper)
    if kind == "nonfinite":
        return _nonfinite(n)
    if kind == "padding":
        return _padding(n)
    if kind == "counts":
        return _counts(n)
    raise KeyError(kind)


def later_gradients(kind, n, step):
    """(packed, grad32, counts) of step 2, 3, ... of a multi-step run of `lanes` or `magnitudes`: new values and another set of visible Gaussians."""
    if kind == "lanes":
        packed, g32 = lanes_gradients(n)
        packed, g32 = np.roll(packed, 17 * step, axis=0), np.roll(g32, 17 * step, axis=0)
    else:
        c = _magnitudes(n, seed=100 + step)
        packed, g32 = c.packed, c.grad32
    return np.ascontiguousarray(packed), np.ascontiguousarray(g32), np.roll(mixed_counts(n), step)


# ----------------------------------------------------------------------------- point cloud rows
def sh_rows(n):
    """u32[n,24]: 48 distinct fp16 bit patterns per Gaussian, none of them a pattern of its neighbours.  Word 1's high half -- the neighbour of the
    third trained half -- is a NaN with a payload on every fifth row, an infinity or a subnormal on others."""
    idx, half = np.arange(n, dtype=np.uint32)[:, None], np.arange(48, dtype=np.uint32)[None, :]
    bits = ((0x0400 + idx * 48 + half) % 0x7800 + ((idx + half) % 2) * 0x8000).astype(np.uint16)
    special = np.array([0x7E55, 0xFC00, 0x0001, 0xFD01, 0x7C00], np.uint16)
    rows = np.arange(n)
    pick = rows % 5 == 0
    bits[pick, 3] = special[(rows[pick] // 5) % special.size]
    return np.ascontiguousarray(bits).view(np.uint32).reshape(n, 24)


def unpack_cloud(n):
    """(gaussians u32[n,6], sh u32[n,24]) where the 12 Gaussian halves and 48 SH halves of a Gaussian are distinct fp16 values, with subnormals,
    +-max, +-0 and +-inf among them (rotating through the halves, so each half position meets each)."""
    idx, half = np.arange(n, dtype=np.uint32)[:, None], np.arange(60, dtype=np.uint32)[None, :]
    bits = ((0x0800 + idx * 60 + half) % 0x7000 + 0x0400 + ((idx + half) % 2) * 0x8000).astype(np.uint16)
    special = np.array([0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x03FF], np.uint16)
    for r in range(n):
        at = (r * 7 + np.arange(special.size) * 6) % 60
        bits[r, at] = special
    g = np.ascontiguousarray(bits[:, :12]).view(np.uint32).reshape(n, 6)
    sh = np.ascontiguousarray(bits[:, 12:]).view(np.uint32).reshape(n, 24)
    return g, sh


def random_rows(n, seed=3):
    """u32[n,8] of random bits: what another rank might publish (word 7's high half is not zero)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    rows[:, 7] |= np.uint32(0x00010000)
    return rows


def skip_windows(n):
    return [(0, 0), (0, n), (0, 1), (n - 1, 1), (255, 2), (256, 256), (900, 0xFFFFFFFF), (0xFFFFFFF0, 0x20), (n, 5)]


RANGES = [(0, 1000), (0, 1), (999, 1), (255, 2), (256, 256), (257, 743), (300, 0)]


def in_window(n, first, count):
    """idx - first < count in wrapping u32 arithmetic, for idx >= first: the window test of apply_rows."""
    idx = np.arange(n, dtype=np.int64)
    return (idx >= first) & (idx - first < count)


# ----------------------------------------------------------------------------- gradient views (store + accumulate)
def gradient_views(n):
    """Three views' (packed block with garbage padding, counts).  Values span the finite fp16 range, so the f32 sums round.  By idx % 16:
    1 -> lane idx % 14 is +inf in view 0 and -inf in view 1 (NaN sum); 2 -> -0 in view 0, +0 in view 1, view 2 not visible (+0 sum);
    3 -> x in view 0, -x in view 1, view 2 not visible (exactly 0); the counts of the other Gaussians are drawn from COUNT_VALUES."""
    views = []
    idx = np.arange(n)
    for v in range(3):
        rng = np.random.default_rng(7000 + v)
        row = halves_of(pack_halves(random_finite_halves(rng, n))).copy()
        views.append([row, COUNT_VALUES[rng.choice([0, 0, 0, 1, 2, 3, 4], n)]])     # zero three times in seven: every number of visible views occurs
    used = np.array(USED_HALVES)
    for i in idx:
        lane = used[i % 14]
        if i % 16 == 1:
            views[0][0][i, lane], views[1][0][i, lane] = 0x7C00, 0xFC00
            views[0][1][i], views[1][1][i], views[2][1][i] = 1, 7, COUNT_VALUES[i % 5]
        elif i % 16 == 2:
            views[0][0][i, used], views[1][0][i, used] = 0x8000, 0x0000
            views[0][1][i], views[1][1][i], views[2][1][i] = 0xFFFFFFFF, 1, 0
        elif i % 16 == 3:
            views[1][0][i, used] = views[0][0][i, used] ^ 0x8000
            views[0][1][i], views[1][1][i], views[2][1][i] = 1, 0x80000000, 0
    return [(garbage_padding(row.view(np.uint32).reshape(n, 8), shift=v), np.ascontiguousarray(c, np.uint32)) for v, (row, c) in enumerate(views)]


def gradient_sums(unpacked, counts, acc=None, visible=None):
    """The store (first view, unless acc / visible are given) and accumulate reference: sequential f32 adds per Gaussian, views in order.
    unpacked: list of f32[n,14]; counts: list of u32[n].  Returns (sums f32[n,14], visible u32[n])."""
    first = acc is None
    for g, c in zip(unpacked, counts):
        vis = (np.asarray(c) != 0)
        g = np.asarray(g, np.float32)
        if first:
            acc = np.where(vis[:, None], g, np.float32(0.0)).astype(np.float32)
            visible = vis.astype(np.uint32)
            first = False
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                acc = np.where(vis[:, None], acc + g, acc).astype(np.float32)
            visible = (visible + vis.astype(np.uint32)).astype(np.uint32)
    return acc, visible


def trained_halves(gaussians, sh):
    """The 14 re-packed fp16 halves of each Gaussian in lane order, u16[n,14]: Gaussian halves 0..10, then SH halves 0, 1, 2."""
    g = np.ascontiguousarray(gaussians).view(np.uint16).reshape(-1, 12)
    s = np.ascontiguousarray(sh).view(np.uint16).reshape(-1, 48)
    return np.concatenate([g[:, :11], s[:, :3]], axis=1)
