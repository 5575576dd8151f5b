"""Hand-built exact nets at the EDGES of the tower formats, beside tests/net_exact.py (whose integer nets live in the
comfortable middle): subnormal activations and weights and the rounding ties around them ("small"), the largest finite
values and the value one f32 ulp below the overflow tie ("large"), activations that reach the overflow tie and go beyond
it from finite weights ("overflow": infinities and NaNs then travel through the tower), and a value head whose argument
walks over zeros, subnormals, large numbers, infinities and a NaN ("value").

Every weight, shift and activation is a power of two or a short sum of them, and check_preconditions asserts on exactly
the boards used that every accumulator is order-independent in f32:
  * all terms finite, sum |terms| below the f32 range: the terms are multiples of a common quantum q with
    sum |terms| / q < 2^24, so every partial sum in any order is exact;
  * all terms finite, the sum beyond the f32 range: the terms have one sign and q >= 2^104, so the partial sums grow
    monotonically, are exact below 2^128 and overflow to that sign's infinity in any order;
  * an infinite term of one sign: the finite terms together stay below 2^127, so no partial sum reaches the other infinity;
  * a NaN term (0 * inf, or a NaN activation) or infinite terms of both signs: NaN in any order.
A tower in any dtype must therefore equal oracle.net_oracle.forward_lowp class for class (finite, +inf, -inf, NaN) and,
within the finite class, bit for bit.

One family of nets per format, generic in the format's constants (net_oracle.FORMAT_LIMITS): N the smallest normal, S
the smallest subnormal, M the largest finite value, P the largest power of two, TIE the overflow tie M + ulp / 2 (65520 in
f16; in f32 the tie is no f32 number and the accumulator itself overflows at 2^128)."""
import functools

import numpy as np

from oracle import net_oracle
from tests import net_exact as ne
from tests.net_compare import classes

EXACT = 2 ** 24
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103            # a float64 sum at or above this is an infinite f32
PRECISION = {"f32": 24, "bf16": 8, "f16": 11}
ONE_VAR = ne.VAR_FOR_SCALE[1.0]                   # every batch-norm scale of these nets is exactly 1
TAPS = [(i, j) for i in range(3) for j in range(3)]
CENTER = (1, 1)
FORMATS = ("bf16", "f16", "f32")


class Consts:
    def __init__(self, fmt):
        self.fmt = fmt
        self.N, self.S, self.M = net_oracle.FORMAT_LIMITS[fmt]
        self.P = 2.0 ** np.floor(np.log2(self.M))
        self.U32 = self.P * 2.0 ** -23                            # one f32 ulp just below the tie
        self.TIE = self.M + self.P * 2.0 ** -PRECISION[fmt]       # (not an f32 number for fmt f32)
        self.H = self.S / 2 if fmt != "f32" else None             # half the smallest subnormal: an f32 number for 16 bits


# ---------------------------------------------------------------- boards

def single_piece_boards():
    """49 boards: one piece of the side to move on square k, nothing else"""
    return np.array([(1 << k, 0) for k in range(49)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def boards():
    """net_exact.edge_boards() and the 49 single-piece boards: 78"""
    return np.concatenate([ne.edge_boards(), single_piece_boards()])


# ---------------------------------------------------------------- building blocks

class Net:
    """the arrays of a net in model.py's layout, filled in entry by entry; every batch-norm scale is 1"""

    def __init__(self, blocks, filters):
        F = filters
        self.blocks, self.F = blocks, F
        self.w = [np.zeros((3, 3, 4, F), np.float64)] + [np.zeros((3, 3, F, F), np.float64) for _ in range(2 * blocks)]
        self.shift = [np.zeros(F, np.float64) for _ in range(2 * blocks + 1)]
        self.hp = np.zeros((1, 1, F, 17), np.float64)
        self.hv = np.zeros((1, 1, F, 1), np.float64)
        self.fc_w = np.zeros((49, 1), np.float32)
        self.fc_b = np.zeros(1, np.float32)

    def first(self, c, shift=0.0, ones=(), mover=(), opp=(), wall=()):
        """channel c of the first layer: the shift and (tap, weight) lists on the four input planes"""
        self.shift[0][c] = shift
        for plane, entries in enumerate((ones, mover, opp, wall)):
            for (i, j), v in entries:
                self.w[0][i, j, plane, c] += v

    def arrays(self):
        f32 = lambda a: np.asarray(a, np.float32)
        for a in self.w + self.shift + [self.hp, self.hv]:
            assert (f32(a).astype(np.float64) == a).all(), "a weight or shift of the net is no f32 number"
        conv = [f32(a) for a in self.w] + [f32(self.hp), f32(self.hv), self.fc_w, self.fc_b]
        bn = []
        for sh in self.shift:
            bn += [f32(-sh), np.full(self.F, ONE_VAR, np.float32)]
        return conv, bn


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _tap(rng):
    return TAPS[int(rng.integers(9))]


def _unit_first(net, c, k, halves=True):
    """a first-layer channel of small integers (the "unit" class): 0 .. 3 depending on the planes around the cell"""
    t1, t2 = TAPS[k % 9], TAPS[(k // 3 + 4) % 9]
    menu = [dict(mover=[(t1, 1.0)], opp=[(t2, 2.0)]), dict(shift=1.0, mover=[(t1, -1.0)], opp=[(t2, 1.0)]),
            dict(mover=[(t1, 2.0)], wall=[(t2, 1.0)]), dict(ones=[(t1, 1.0)], mover=[(t2, 1.0)])]
    if halves:
        menu.append(dict(shift=0.5, mover=[(t1, 1.0)], opp=[(t2, -0.5)]))
    net.first(c, **menu[k % len(menu)])


def _unit_conv(net, layer, o, rng, units, halves=True):
    """an output channel of the unit class: small integers (and halves) from unit channels"""
    for c in rng.choice(units, size=3, replace=False):
        net.w[layer][_tap(rng) + (int(c), o)] += _pick(rng, [1.0, -1.0, 0.5, -0.5] if halves else [1.0, -1.0, 1.0, -1.0])
    net.shift[layer][o] = _pick(rng, [0.0, 1.0, -1.0, 0.5] if halves else [0.0, 1.0, -1.0, 0.0])


def _value_head(net, features, fmt, channels, rng, arg_top=1.5):
    """the value 1x1 convolution on `channels` (+-1) and fc weights j * 2^-k that keep the argument within +-arg_top"""
    for c in channels:
        net.hv[0, 0, c, 0] = _pick(rng, [1.0, -1.0])
    conv, bn = net.arrays()
    h = trace(conv, bn, features, fmt)[-1]["a"]
    vcell = (np.where(np.isfinite(h), h, 0.0) @ net.hv[0, 0])[..., 0].reshape(len(h), 49)
    j = (rng.integers(1, 4, size=49) * rng.choice([-1, 1], size=49)).astype(np.float64)
    top = max(np.abs(vcell * j).sum(axis=1).max(), 2.0 ** -140)
    k = max(int(np.ceil(np.log2(top / arg_top))), -120)       # (fc weights stay f32 numbers: tiny arguments then)
    net.fc_w = (j * 2.0 ** -k).astype(np.float32).reshape(49, 1)
    net.fc_b = np.array([rng.integers(-5, 6) * 2.0 ** -4], np.float32)


# ---------------------------------------------------------------- the "small" family

def small_net(blocks, filters, fmt, seed=1):
    """Classes: T ("tiny", the first 3/4 of the channels: multiples of S up to a few N) and U ("unit": small integers).
    T outputs sum T inputs under weights 1, -1, 2 (and 1/2 in the 16-bit formats: odd multiples of S / 2 are the ties)
    and U inputs under weights that are subnormal, or the smallest normal, in the format."""
    K = Consts(fmt)
    N, S, H = K.N, K.S, K.H
    rng = np.random.default_rng(seed)
    F = filters
    nT = 3 * F // 4
    T, U = np.arange(nT), np.arange(nT, F)
    net = Net(blocks, F)
    TN = T[:0]
    if fmt == "f32":
        # N is 2^23 S: two values near it in one f32 accumulator are no longer exact.  Three channels hold N - S, N and
        # N + S and only ever feed accumulators of one term (themselves again, through the block; three logits); the
        # other channels stay below 2^12 S.
        TN, T, N = T[:3], T[3:], 2.0 ** 12 * S
        net.first(0, mover=[(CENTER, K.N)], opp=[(CENTER, -K.N)])
        net.first(1, shift=K.N - S, mover=[((0, 1), S)], opp=[((2, 1), -(K.N - S))])
        net.first(2, shift=S, mover=[((1, 2), K.N - S)], ones=[((1, 0), S)])
    for c in T:
        t1, t2, t3 = TAPS[c % 9], TAPS[(c // 9 + 4) % 9], TAPS[(c // 2 + 1) % 9]
        menu = [dict(mover=[(t1, N)], opp=[(t2, -N)]),                                 # the smallest normal
                dict(mover=[(t1, N - S)], opp=[(t2, -(N - S))]),                       # 1 ulp below: all fraction bits set
                dict(mover=[(t1, S)], opp=[(t2, -S)]),                                 # the smallest subnormal
                dict(shift=S, mover=[(t1, N - S)], ones=[(t3, S)]),                    # S, 2 S, N, N + S: edge dependent
                dict(mover=[(t1, 2 * N)], opp=[(t2, -2 * N)], wall=[(t3, S)]),
                dict(shift=N - S, mover=[(t1, S)], opp=[(t2, -(N - S))])]              # N - S, N, +0
        if H:
            menu += [dict(shift=H, mover=[(t1, S)], opp=[(t2, -S)]),                   # S/2 -> 0, 3 S/2 -> 2 S, -S/2 -> -0
                     dict(shift=-H, mover=[(t1, 2 * S)], opp=[(t2, S)]),               # -S/2 -> -0, 3 S/2 -> 2 S, S/2 -> 0
                     dict(shift=H, mover=[(t1, N - S)], ones=[(t3, S)])]               # N - S/2: the tie below N, up to N
        net.first(int(c), **menu[c % len(menu)])
    for k, c in enumerate(U):
        _unit_first(net, int(c), k, halves=fmt != "f32")        # (f32: a half times a subnormal weight is no f32 number)
    w_tt = [1.0, -1.0, 2.0, 1.0, -1.0] + ([0.5, -0.5, 0.5] if H else [])
    w_ut = [S, -S, N, -N, N - S, 2 * S, 3 * S, -(N - S)]
    sh_t = [0.0, S, -S, -N, 0.0] + ([H, -H, 3 * H] if H else [])
    for layer in range(1, 2 * blocks + 1):
        for o in TN:
            if layer % 2 == 1:
                net.w[layer][CENTER + (int(o), int(o))] = 1.0      # (a block's second conv: the residual input alone)
        for o in T:
            for c in rng.choice(T, size=2, replace=False):
                net.w[layer][_tap(rng) + (int(c), int(o))] += _pick(rng, w_tt)
            for c in rng.choice(U, size=2, replace=False):
                net.w[layer][_tap(rng) + (int(c), int(o))] += _pick(rng, w_ut)
            net.shift[layer][o] = _pick(rng, sh_t)
        for o in U:
            _unit_conv(net, layer, int(o), rng, U, halves=fmt != "f32")
    for o in range(17):
        if o < len(TN):
            net.hp[0, 0, TN[o], o] = _pick(rng, [1.0, -1.0])
            continue
        for c in rng.choice(T, size=4, replace=False):
            net.hp[0, 0, c, o] = _pick(rng, [1.0, -1.0, 2.0, 4.0, -2.0])
    _value_head(net, ne.features(boards()), fmt, rng.choice(T, size=2, replace=False), rng)
    return net.arrays()


# ---------------------------------------------------------------- the "large" and "overflow" families

def large_net(blocks, filters, fmt, seed=2, overflow=False):
    """Classes: BM (4 channels that hold M; they only ever feed accumulators of one term, because M has all the
    format's bits), BO (4 channels, overflow nets only: they reach TIE and beyond where the mover has pieces), BP (values
    around P, the largest power of two), the indicator channel of the mover's pieces (kept alive by the residual path, so
    that a folded weight of M meets an activation of 1 in every block) and U (small integers).
    overflow: the BO channels are fed from the mover's plane only, so cells away from the mover's pieces stay finite: a
    net without blocks overflows in the 3x3 neighbourhood of a piece, a net with blocks on the piece's cell, and every
    layer after that carries the infinities and NaNs one cell further."""
    K = Consts(fmt)
    N, S, M, P, TIE, U32 = K.N, K.S, K.M, K.P, K.TIE, K.U32
    f32fmt = fmt == "f32"
    rng = np.random.default_rng(seed)
    F = filters
    BM, BO = np.arange(0, 4), np.arange(4, 8)
    BP = np.arange(8, F // 4)
    IND = F // 4
    U = np.arange(F // 4 + 1, F)
    net = Net(blocks, F)
    # first layer
    net.first(0, mover=[(CENTER, M)], opp=[(CENTER, -M)])                               # a folded weight of M
    net.first(1, shift=M - P, mover=[((0, 1), P)])                                      # M as a sum of two terms
    if f32fmt:
        net.first(2, mover=[((2, 1), M)])
    else:
        net.first(2, shift=TIE - U32 - P, mover=[((2, 1), P)])                          # 1 f32 ulp below the tie: rounds to M
    net.first(3, shift=M, mover=[] if f32fmt else [(CENTER, -P)])                       # M everywhere (16 bits: but on the pieces)
    if overflow:
        near = TAPS if blocks == 0 else [CENTER]
        if f32fmt:
            net.first(4, shift=P, mover=[(t, P) for t in near])                         # 2^128: the accumulator overflows
        else:
            net.first(4, shift=TIE - P, mover=[(t, P) for t in near])                   # exactly the tie (one piece), beyond
        if f32fmt:
            net.first(5, shift=1.75 * P, mover=[(CENTER, P)])                           # (M only where it is the one term)
        else:
            net.first(5, shift=M, mover=[(CENTER, M)])                                  # 2 M
        net.first(6, shift=1.5 * P, mover=[(CENTER, P)] + ([((0, 1), P)] if blocks == 0 else []))
        net.first(7, shift=P / 2, mover=[(CENTER, 1.5 * P)])
    for k, c in enumerate(BP):
        t1, t2 = TAPS[k % 9], TAPS[(k // 2 + 3) % 9]
        menu = [dict(mover=[(t1, P)], opp=[(t2, -P)]), dict(shift=P / 2, mover=[(t1, P / 2)], opp=[(t2, -P / 2)]),
                dict(shift=P / 4, ones=[(t1, P / 4)], mover=[(t2, P / 2)]), dict(opp=[(t1, P)], wall=[(t2, P / 2)])]
        net.first(int(c), **menu[k % len(menu)])
    net.first(IND, mover=[(CENTER, 1.0)])
    for k, c in enumerate(U):
        _unit_first(net, int(c), k)
    # (f32 keeps every bit from layer to layer: one exponent, so that the quantum shrinks by 2^-3 a layer and no faster)
    small_w = [2.0 ** -3, -2.0 ** -3] + ([2.0 ** -4, -2.0 ** -4] if not f32fmt else [])
    # 1 / P is a subnormal weight in every format (2^-15 in f16); N the smallest normal weight
    down_w = [1.0 / P, -1.0 / P, 2.0 / P, N]
    for layer in range(1, 2 * blocks + 1):
        second = layer % 2 == 0
        for o in BM:
            if not second:
                if o % 2 == 0:
                    net.w[layer][CENTER + (IND, int(o))] = M                            # M * 1 on the mover's pieces
                else:
                    net.w[layer][CENTER + (int(o), int(o))] = 0.5                       # M / 2
            # (second conv: no weights, the residual input passes through alone)
        if overflow:
            for o in BO:
                if second:
                    continue
                # on the overflowing channels of its input: all nine taps positive (+inf around a piece), all negative
                # (-inf into the ReLU) or nothing (0 * inf: a NaN)
                kind = (o - 4) % 3
                for c in BO:
                    for t in TAPS:
                        if kind < 2:
                            net.w[layer][t + (int(c), int(o))] = 2.0 ** -7 if kind == 0 else -2.0 ** -7
        for o in BP:
            srcs = rng.choice(BP, size=3, replace=False)
            for c in srcs:
                w = _pick(rng, small_w)
                net.w[layer][_tap(rng) + (int(c), int(o))] += -abs(w) if second else w
            if overflow and o % 3 == 0 and not second:
                for c in BO:
                    for t in TAPS:
                        net.w[layer][t + (int(c), int(o))] = 2.0 ** -8 * (1 if o % 2 else -1)
            net.shift[layer][o] = 0.0 if second else _pick(rng, [0.0, P / 4, -P / 8, P / 8])
        # (the indicator channel: no weights in either conv — zero after a block's first conv, itself again after the second)
        for o in U:
            _unit_conv(net, layer, int(o), rng, U)
            if o % 4 == 0:
                c = int(_pick(rng, BP))
                net.w[layer][_tap(rng) + (c, int(o))] += _pick(rng, down_w)             # a large activation, a tiny weight
    for o in range(17):
        if o < 4:
            net.hp[0, 0, BM[o], o] = _pick(rng, [2.0 ** -3, -2.0 ** -4])                # one term: M has every bit
        else:
            for c in rng.choice(BP, size=3, replace=False):
                net.hp[0, 0, c, o] = _pick(rng, small_w) * 2.0 ** -3
            net.hp[0, 0, _pick(rng, U), o] += _pick(rng, [P * 2.0 ** -8, -P * 2.0 ** -8])
        if overflow and o >= 4:
            # +inf, -inf or (no weight on the overflowing channels: 0 * inf) a NaN around the mover's pieces
            kind = o % 3
            if kind < 2:
                net.hp[0, 0, BO, o] = 2.0 ** -6 if kind == 0 else -2.0 ** -6
    _value_head(net, ne.features(boards()), fmt, rng.choice(U, size=2, replace=False), rng)
    return net.arrays()


def overflow_net(blocks, filters, fmt, seed=3):
    return large_net(blocks, filters, fmt, seed, overflow=True)


# ---------------------------------------------------------------- the value head

NAN32 = np.float32(np.nan)
VALUE_ENTRIES = [0.0, -0.0, 2.0 ** -149, -3 * 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -20, -2.0 ** -20, 0.5, -0.5, 8.0, -8.0,
                 9.1, -9.1, 20.0, -20.0, 88.0, -88.0, 2.0 ** 100, -2.0 ** 100, 1.5, -1.5, 1.0, 0.25, 3.0, -3.0, 5.0, 2.0 ** -12,
                 2.0 ** -10, 2.0 ** -130, 0.75, -0.125]
VALUE_CELL = 24                                    # the square of the non-finite fc weight: x = 3, y = 3
VALUE_KINDS = ("finite", "pinf", "ninf", "nan")


def value_net(kind, fmt):
    """A net without blocks whose value convolution sees 1 on the mover's pieces (kind "finite"): on a single-piece board
    the argument of tanh is one fc_w entry plus fc_b (0 here, so that -0 and the subnormals arrive as they are), and the 49
    entries walk over VALUE_ENTRIES.  The other kinds put +inf, -inf or a NaN at fc_w[VALUE_CELL] and let the value
    convolution see the 3x3 neighbourhood of the pieces as well, with either sign — the route of helpers.nonfinite_net: the
    argument is +-inf where that cell's activation is not 0 and a NaN where it is 0."""
    assert kind in VALUE_KINDS
    net = Net(0, 128)
    net.first(0, mover=[(CENTER, 1.0)])
    net.first(1, mover=[(t, 1.0) for t in TAPS if t[1] != 1 or t == CENTER])          # the piece, and its x neighbours' rows
    net.first(2, mover=[(t, 1.0) for t in TAPS if t[1] == 1 and t != CENTER])
    for c in range(3, 128):
        _unit_first(net, c, c)
    rng = np.random.default_rng(7)
    for o in range(17):
        for c in rng.choice(np.arange(3, 128), size=3, replace=False):
            net.hp[0, 0, c, o] = _pick(rng, [1.0, -1.0, 2.0])
    net.hv[0, 0, 0, 0] = 1.0
    entries = (VALUE_ENTRIES * 2)[:49]
    net.fc_w = np.array(entries, np.float32).reshape(49, 1)
    if kind != "finite":
        net.hv[0, 0, 1, 0], net.hv[0, 0, 2, 0] = 1.0, -2.0
        net.fc_w[VALUE_CELL, 0] = {"pinf": np.inf, "ninf": -np.inf, "nan": NAN32}[kind]
    return net.arrays()


# ---------------------------------------------------------------- the trace and the preconditions

def _quantum(a):
    """the largest power of two that divides every non-zero finite entry of a (inf for none)"""
    a = np.abs(np.asarray(a, np.float64))
    a = a[np.isfinite(a) & (a > 0)]
    if not a.size:
        return np.inf
    m, e = np.frexp(a)
    low = np.array([(int(x) & -int(x)) for x in (m * 2.0 ** 53).astype(np.int64)], dtype=np.float64)   # lowest set bit
    return float((low * 2.0 ** (e.astype(np.float64) - 53)).min())


def _channel_quanta(a):
    return np.array([_quantum(a[..., c]) for c in range(a.shape[-1])])


def _accumulators(x, w, const, const_q):
    """The accumulators sum_taps x * w + const of one layer (x (n,7,7,cin) >= 0 or not finite, w (k,k,cin,cout) finite,
    const (n,7,7,cout) or (cout,): shift and residual), classified by their TERMS and checked for order independence
    -> (expected class (n,7,7,cout), exact float64 sum of the finite terms)."""
    conv = net_oracle.conv2d_same
    assert np.isfinite(w).all()
    fin = np.where(np.isfinite(x), x, 0.0)
    assert (fin >= 0).all()
    is_inf, is_nan = (x == np.inf).astype(np.float64), np.isnan(x).astype(np.float64)
    ones = np.ones_like(w)
    nan_terms = conv(is_nan, ones) + conv(is_inf, (w == 0).astype(np.float64))
    pinf_terms = conv(is_inf, (w > 0).astype(np.float64))
    ninf_terms = conv(is_inf, (w < 0).astype(np.float64))
    const = np.broadcast_to(const, nan_terms.shape)
    nan_terms = nan_terms + np.isnan(const)
    pinf_terms = pinf_terms + (const == np.inf)
    const_fin = np.where(np.isfinite(const), const, 0.0)
    pos = conv(fin, np.maximum(w, 0)) + np.maximum(const_fin, 0)
    neg = conv(fin, np.maximum(-w, 0)) + np.maximum(-const_fin, 0)
    assert (fin.max(axis=(0, 1, 2)) * np.abs(w).max(axis=(0, 1, 3))).max() < F32_OVERFLOW, "a single product overflows f32"
    total, bound = pos - neg, pos + neg
    # the common quantum of an output channel's terms: products of its input channels' quanta with its weights', and the constants'
    qa = _channel_quanta(fin)
    q = np.full(w.shape[-1], np.inf)
    for o in range(w.shape[-1]):
        for c in np.nonzero(np.abs(w[..., o]).sum(axis=(0, 1)))[0]:
            if np.isfinite(qa[c]):
                q[o] = min(q[o], qa[c] * _quantum(w[:, :, c, o]))
    q = np.minimum(q, const_q)
    assert q.min() >= 2.0 ** -149, "a term is no f32 number"
    expected = np.where((nan_terms > 0) | ((pinf_terms > 0) & (ninf_terms > 0)), 3,
                        np.where(pinf_terms > 0, 1, np.where(ninf_terms > 0, 2, 0)))
    span = np.maximum(pos, neg)                   # every partial sum of the finite terms, in any order, lies in [-neg, pos]
    has_inf = (pinf_terms + ninf_terms > 0) & (expected != 3)
    assert (span[has_inf] <= 1.5 * 2.0 ** 127).all(), "finite terms beside an infinite one could overflow on their own"
    plain = expected == 0
    small = plain & (span < F32_OVERFLOW)
    ratio = np.where(small, bound, 0.0) / np.where(np.isfinite(q), q, 1.0)
    assert ratio.max() < EXACT, ("sum |terms| / quantum reaches 2^24", float(ratio.max()))
    big = plain & ~small
    if big.any():
        assert ((pos == 0) | (neg == 0))[big].all(), "terms of both signs in an accumulator that may overflow"
        assert (np.broadcast_to(q, bound.shape)[big] >= 2.0 ** 104).all(), "partial sums below 2^128 would not be exact"
        expected = np.where(big & (np.abs(total) >= F32_OVERFLOW), np.where(total > 0, 1, 2), expected)
    return expected, total


def trace(conv, bn, features, fmt, check=False, erase_nan=False):
    """The tower layer by layer as the emulator computes it -> [dict(z pre-activation in the format (after rounding),
    acc the f32 accumulator, a activation)], from lowp_parameters and conv2d_same.  check: every accumulator's terms are
    classified and checked for order independence (_accumulators), and the class they imply is the class computed."""
    layers = net_oracle.lowp_parameters(conv, bn, fmt)[0]
    rnd = net_oracle._rounder(fmt)
    h = np.asarray(features, np.float64)
    out, t = [], None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (w, shift) in enumerate(layers):
            w, shift = w.astype(np.float64), shift.astype(np.float64)
            second = i > 0 and i % 2 == 0
            inp = t if second else h
            acc = net_oracle.conv2d_same(inp, w) + shift
            if second:
                acc = acc + h
            acc = acc.astype(np.float32)
            z = rnd(acc).astype(np.float64)
            a = np.maximum(z, 0)
            if erase_nan:                       # the ReLU of the bf16 16x16x32 towers: a NaN becomes 0 (net_oracle, the
                a = np.where(np.isnan(a), 0.0, a)   # defect relu_erases_negative_nan_only)
            if check:
                const = shift + h if second else shift
                const_q = np.minimum(_channel_quanta(shift[None]), _channel_quanta(np.where(np.isfinite(h), h, 0))) if second \
                    else _channel_quanta(shift[None])
                expected, total = _accumulators(inp, w, const, const_q)
                assert (classes(acc) == expected).all(), "layer %d: the terms' class is not the emulator's" % i
                ok = expected == 0
                assert (acc.astype(np.float64)[ok] == total[ok]).all(), "layer %d: an accumulator is not exact" % i
            out.append(dict(z=z, acc=acc.astype(np.float64), a=a))
            if i % 2 == 1:
                t = a
            else:
                h = a
    return out


def count_ties(acc, fmt):
    """accumulators that are exact rounding ties of the format (positive or negative)"""
    if fmt == "f32":
        return 0
    x = np.abs(acc[np.isfinite(acc) & (acc != 0)]).astype(np.float32)
    below = net_oracle._truncate_bf16(x) if fmt == "bf16" else net_oracle._truncate_f16(x)
    inexact = below != x
    x, below = x[inexact].astype(np.float64), below[inexact].astype(np.float64)
    K = Consts(fmt)
    ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(below, K.S))) - (PRECISION[fmt] - 1)), K.S)
    ulp = np.where(below == 0, K.S, ulp)
    return int((x - below == ulp / 2).sum())


def check_preconditions(family, conv, bn, fmt, feats=None):
    """Assert what makes the net an exact test of the `fmt` tower on exactly the boards used (both masks), and what its
    family promises.  -> statistics"""
    K = Consts(fmt)
    feats = ne.features(boards()) if feats is None else feats
    rnd = net_oracle._rounder(fmt)
    layers, head_p, head_v, fc_w, fc_b = net_oracle.lowp_parameters(conv, bn, fmt)
    blocks = (len(layers) - 1) // 2
    for i, (w, shift) in enumerate(layers):
        assert np.isfinite(w).all() and np.isfinite(shift).all()
        assert (w == conv[i]).all(), "layer %d: a folded weight is not the weight written down" % i
        assert (shift == -np.asarray(bn[2 * i], np.float32)).all(), "layer %d: a shift is not the one written down" % i
    tr = trace(conv, bn, feats, fmt, check=True)
    with np.errstate(invalid="ignore", over="ignore"):
        p, v, acts, arg = net_oracle._forward_lowp(conv, bn, feats, fmt, with_argument=True)
    for i, (layer, a) in enumerate(zip(tr, acts)):
        assert np.array_equal(layer["a"], a, equal_nan=True), "layer %d: the trace is not the emulator" % i
    h = tr[-1]["a"]
    # the heads: the same rule, one 1x1 "layer" of 18 outputs from zero accumulators
    if family != "value":
        assert np.isfinite(head_p).all() and np.isfinite(head_v).all()
        hw = np.concatenate([head_p, head_v.reshape(-1, 1)], axis=1).astype(np.float64)[None, None]
        expected, total = _accumulators_1x1(h, hw)
        got = np.concatenate([p, acts_value_cells(h, head_v)[..., None]], axis=-1)
        assert (classes(got) == expected).all()
        assert (got[expected == 0] == total[expected == 0]).all(), "a head accumulator is not exact"
    stats = dict(family=family, fmt=fmt, blocks=blocks, logit_classes=[float((classes(p) == k).mean()) for k in range(4)],
                 ties=sum(count_ties(layer["acc"], fmt) for layer in tr))
    n = len(feats)
    board_cls = classes(p).reshape(n, -1)
    stats["boards_all_finite"] = int((board_cls == 0).all(axis=1).sum())
    stats["boards_nan_and_finite"] = int(((board_cls == 3).any(axis=1) & (board_cls == 0).any(axis=1)).sum())
    if family == "small":
        assert np.isfinite(p).all() and np.isfinite(v).all()
        shares = []
        for i, layer in enumerate(tr):
            a = layer["a"]
            nz = a[a > 0]
            share = float((nz < K.N).mean())
            shares.append(share)
            assert share >= 0.05, ("layer %d: %.3f of the non-zero activations are subnormal" % (i, share))
        stats["subnormal_share"] = shares
        accs = np.concatenate([layer["acc"].ravel() for layer in tr])
        # (-0 comes from rounding a tiny negative accumulator; the f32 tower does not round)
        assert fmt == "f32" or (np.signbit(accs) & (accs == 0)).any() or any(
            (np.signbit(layer["z"]) & (layer["z"] == 0)).any() for layer in tr), "-0 never occurs as a pre-activation"
        assert any((layer["z"] < 0).any() for layer in tr) and any((layer["z"] > 0).any() for layer in tr)
        if fmt != "f32":
            assert stats["ties"] >= 20, stats
        assert np.unique(p).size >= 100, ("the logits are not distinct enough to tell boards and cells apart", np.unique(p).size)
        a0 = tr[0]["a"]
        for x in [K.N, K.N - K.S, K.S] + ([2 * K.S] if K.H else []):
            assert (a0 == x).any(), x
        if K.H:
            for x in (K.H, 3 * K.H, -K.H):
                assert (tr[0]["acc"] == x).any(), x
    if family == "large":
        assert np.isfinite(p).all() and np.isfinite(v).all()
        for i, layer in enumerate(tr):
            assert np.isfinite(layer["a"]).all()
        assert all((layer["a"] == K.M).any() for layer in tr), "M is not reached in every layer"
        assert max(np.abs(w).max() for w, _ in layers) == K.M
        if fmt != "f32":
            assert (tr[0]["acc"] == K.TIE - K.U32).any() and (tr[0]["acc"] != tr[0]["z"]).any()
        assert np.unique(p).size >= 30, np.unique(p).size
    if family == "overflow":
        cls = stats["logit_classes"]
        assert stats["boards_all_finite"] >= 1, stats
        a0 = tr[0]
        if fmt != "f32":
            assert (a0["acc"] == K.TIE).any(), "no accumulator sits exactly on the overflow tie"
        assert (a0["acc"][np.isfinite(a0["acc"])] > K.M).any() or fmt == "f32"
        assert np.isinf(a0["a"]).any()
        # fed from the mover's plane: a board without pieces of the mover stays finite everywhere
        no_mover = feats[..., 1].sum(axis=(1, 2)) == 0
        assert no_mover.any() and (board_cls[no_mover] == 0).all() and np.isfinite(v[no_mover]).all()
        if blocks == 0:
            assert min(cls) >= 0.05, ("each class holds at least 5 % of the logits", cls)
        else:
            assert stats["boards_nan_and_finite"] >= 5, stats
            relu_in = np.concatenate([layer["z"].ravel() for layer in tr[1:]])
            relu_out = np.concatenate([layer["a"].ravel() for layer in tr[1:]])
            assert np.isnan(relu_out).any() and (relu_out == np.inf).any() and (np.isfinite(relu_out) & (relu_out > 0)).any()
            assert (relu_in == -np.inf).any(), "no pre-activation of -inf reaches a ReLU"
    if family == "value":
        stats["value_classes"] = [float((classes(v) == k).mean()) for k in range(4)]
        stats["arguments"] = arg
    return stats


def acts_value_cells(h, head_v):
    with np.errstate(invalid="ignore", over="ignore"):
        return (h @ head_v.astype(np.float64)).astype(np.float32).astype(np.float64)


def _accumulators_1x1(h, hw):
    q0 = np.full(hw.shape[-1], np.inf)
    return _accumulators(h, hw, np.zeros(hw.shape[-1]), q0)


# ---------------------------------------------------------------- the cases of the tests

FAMILIES = {"small": small_net, "large": large_net, "overflow": overflow_net}
SIZES = [(0, 128), (1, 128), (2, 128), (1, 64)]
TOWER_CASES = [(family, blocks, filters, fmt) for family in FAMILIES for blocks, filters in SIZES for fmt in FORMATS]
VALUE_CASES = [("value-" + kind, 0, 128, fmt) for kind in VALUE_KINDS for fmt in FORMATS]
CASES = TOWER_CASES + VALUE_CASES


def case_id(case):
    return "%s-%dx%d-%s" % case


@functools.lru_cache(maxsize=None)
def edge_net(family, blocks, filters, fmt):
    """-> (conv, bn, leaf boards, statistics), the preconditions checked on the boards under both masks"""
    if family.startswith("value-"):
        conv, bn = value_net(family[6:], fmt)
        stats = check_preconditions("value", conv, bn, fmt)
    else:
        conv, bn = FAMILIES[family](blocks, filters, fmt)
        stats = check_preconditions(family, conv, bn, fmt)
    return conv, bn, boards(), stats


@functools.lru_cache(maxsize=None)
def reference(family, blocks, filters, fmt, mask):
    """the emulator on the case's boards under one mask, computed once -> (logits, values, value arguments)"""
    conv, bn, lb, _ = edge_net(family, blocks, filters, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        p, v, _, arg = net_oracle._forward_lowp(conv, bn, net_oracle.features_from_leaf_boards(lb, mask), fmt,
                                                with_argument=True)
    for a in (p, v, arg):
        a.setflags(write=False)
    return p, v, arg


@functools.lru_cache(maxsize=None)
def reference_erased_nan(family, blocks, filters, fmt, mask):
    """What a tower computes whose ReLU clears the NaN the device generates (the emulator's defect
    relu_erases_negative_nan_only: the bf16 16x16x32 towers today), on the case's boards under one mask -> (logits,
    values, value arguments).  With other activations the accumulators have other terms, so their order independence is
    checked again, layer by layer and in the heads, on exactly these boards."""
    conv, bn, lb, _ = edge_net(family, blocks, filters, fmt)
    feats = net_oracle.features_from_leaf_boards(lb, mask)
    tr = trace(conv, bn, feats, fmt, check=True, erase_nan=True)
    with np.errstate(invalid="ignore", over="ignore"):
        p, v, acts, arg = net_oracle._forward_lowp(conv, bn, feats, fmt, defect="relu_erases_negative_nan_only", with_argument=True)
    for layer, a in zip(tr, acts):
        assert np.array_equal(layer["a"], a, equal_nan=True)
    head_p, head_v = net_oracle.lowp_parameters(conv, bn, fmt)[1:3]
    h = tr[-1]["a"]
    hw = np.concatenate([head_p, head_v.reshape(-1, 1)], axis=1).astype(np.float64)[None, None]
    expected, total = _accumulators_1x1(h, hw)
    got = np.concatenate([p, acts_value_cells(h, head_v)[..., None]], axis=-1)
    assert (classes(got) == expected).all() and (got[expected == 0] == total[expected == 0]).all()
    for a in (p, v, arg):
        a.setflags(write=False)
    return p, v, arg


# ---------------------------------------------------------------- helpers.nonfinite_net against the emulator

# A position's classes on helpers.nonfinite_net are decided by the SIGN of a few pre-activations of its last tower layer:
# policy channel 58 at every cell (+inf logit where it is active, NaN where it is not) and the value channel at `cell`
# (+-1 or NaN).  The net is a random one, not an exact one, so a tower and the emulator may disagree on a pre-activation
# that lies within accumulation-order noise of zero.  That noise is bounded through the emulator's own distance D from
# float64 on these very pre-activations (the max over all positions), which is the sum of the 16-bit roundings of 1152
# inputs and weights.  A 16-bit tower differs from the emulator by the f32 summation order (1e-7 relative) and, where that
# noise carries an input of the layer across a rounding boundary, by ONE 16-bit ulp of ONE of the 1152 inputs: |z| < D / 4
# is "too close" — room for several such flips at once.  The f32 tower sums the 1152 terms in f32 where the emulator sums
# them in float64 and rounds once — sqrt(1152) ~ 34 roundings against one — so there |z| < 64 D.
CLOSE_FACTOR = {"bf16": 0.25, "f16": 0.25, "f32": 64.0}
MAX_LEFT_OUT = 0.10
NONFINITE_CELL, NONFINITE_VALUE_CHANNEL, NONFINITE_POLICY_CHANNEL = 4, 64, 58


@functools.lru_cache(maxsize=None)
def hostile_positions():
    """the positions of tests/test_hostile_net.py: twelve random lines from the late start position, as (mover, opponent)"""
    from tests import helpers
    from tests.engine_harness import late_start_fen
    out = []
    for seed in range(12):
        for packed, _, _ in helpers.random_line(late_start_fen(), seed):
            w0, w1 = int(packed[0]), int(packed[1])
            x = w0 & ~(1 << 63)
            out.append((w1, x) if w0 >> 63 else (x, w1))
    return np.array(out, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def nonfinite_reference(fmt):
    """-> dict(boards, p, v: the emulator's logits and values on hostile_positions(); keep: the positions none of whose
    deciding pre-activations lies within tau of zero; tau, distance D, factor)"""
    from tests import helpers
    conv, bn = helpers.nonfinite_net()
    lb = hostile_positions()
    feats = net_oracle.features_from_leaf_boards(lb, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        p, v = net_oracle.forward_lowp(conv, bn, feats, fmt)
    z = trace(conv, bn, feats, fmt)[-1]["acc"]
    cw = [np.asarray(a, np.float64) for a in conv]
    relu_bn = lambda x, i: net_oracle.batch_norm(x, np.asarray(bn[2 * i], np.float64), np.asarray(bn[2 * i + 1], np.float64))
    h0 = np.maximum(relu_bn(net_oracle.conv2d_same(feats, cw[0]), 0), 0)
    t = np.maximum(relu_bn(net_oracle.conv2d_same(h0, cw[1]), 1), 0)
    z64 = relu_bn(net_oracle.conv2d_same(t, cw[2]), 2) + h0
    cx, cy = NONFINITE_CELL // 7, NONFINITE_CELL % 7
    deciding = lambda a: np.concatenate([a[..., NONFINITE_POLICY_CHANNEL].reshape(len(lb), 49),
                                         a[:, cx, cy, NONFINITE_VALUE_CHANNEL].reshape(len(lb), 1)], axis=1)
    d, d64 = deciding(z), deciding(z64)
    dist = float(np.abs(d - d64).max())
    tau = CLOSE_FACTOR[fmt] * dist
    keep = (np.abs(d) >= tau).all(axis=1)
    return dict(boards=lb, p=p, v=v, keep=keep, tau=tau, distance=dist, factor=CLOSE_FACTOR[fmt])
